// genome_pass.cpp -- the host side of --gpu_parse for genome FASTA, shared by ntedit-make-genome-bf and ntedit --genome:
// one pass over the genome files that either inserts every k-mer into a filter slot or only adds up the bases (the
// sizing pass).  A file goes to the device in chunks of batch_bytes raw bytes cut wherever they end -- a chromosome is
// longer than any chunk -- and the stateful grammar (nte_genome_grammar.h) carries what a cut hides: each chunk is
// entered in its predecessor's exit state.  The chunk's text lands behind the last k - 1 text bytes of its file, so the
// k-mers across a cut are in the batch that ntedit_hip_filter_insert gets; insertion is idempotent, so the overlap
// changes no bit.
//
//   plain files   pread into two page-locked buffers by a reader thread (chunk_feed.h: RawProducer, cut anywhere); the
//                 copy of a chunk runs on the copy stream while the chunk before is parsed and inserted (overlap)
//   BGZF files    shipped compressed, in whole members whose ISIZE sum stays within batch_bytes (BgzfGather), and inflated on the
//                 device (ntedit_hip_reads_inflate_device); no cut is looked for, the state carries over
//   hand-back     from the first unclean chunk of a file on the host parser takes the file, from the last record start
//                 known from the clean chunks before it (their last_header), or from offset 0; the sizing pass reads
//                 such a file again from its start, so that no base is counted twice
//   host files    single-stream .gz files and files that do not start with '>' take the host parser whole, and with
//                 batch_bytes 0 every file does (the pass without --gpu_parse)
#include "../csrc/nte_reads_internal.h"
#include "chunk_feed.h"
#include "fasta.h"

#include <chrono>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

namespace {

const uint64_t NO_START = NTEDIT_READS_NO_START;
const size_t HOST_FLUSH = 512u << 20;   // the host parser's batches, as ntedit-make-genome-bf makes them

int
pfail(const ntedit_hip_ctx* c, int code, const std::string& why)
{
	return nte_reads::set_error(c, code, why);
}

// why a feed (chunk_feed.h) gave up: no page-locked memory, or the file
int
feed_fail(const ntedit_hip_ctx* c, const std::string& why)
{
	return pfail(c, why == nte_host::NO_PINNED ? NTEDIT_E_DEVICE : NTEDIT_E_IO, why);
}

struct Pass
{
	ntedit_hip_ctx* ctx;
	int slot, insert;
	uint32_t k = 0;
	uint64_t batch_bytes;
	uint64_t bases = 0;
	double gpu_ms = 0.0;
	ntedit_hip_genome_pass_info* info;

	// one clean chunk's batch through the insert
	int insert_batch(const char* batch, uint64_t text_len)
	{
		if (!insert) {
			return 0;
		}
		int rc = ntedit_hip_filter_insert(ctx, slot, batch, (uint64_t)nte_reads::genome_pad() + text_len, NTEDIT_HIP_BASES_DEVICE);
		if (rc) {
			return pfail(ctx, rc, std::string("filter_insert: ") + ntedit_hip_last_error(ctx));
		}
		return nte_reads::genome_carry(ctx, text_len, k - 1);
	}

	// the host parser over the file from a record start: `begin` a file offset (plain files), `skip` an inflated
	// offset (gzip files)
	int host_parse(const char* path, uint64_t begin, uint64_t skip)
	{
		std::unique_ptr<nte_host::FastaReader> reader(begin ? new nte_host::FastaReader(path, begin, ~0ull)
		                                                    : new nte_host::FastaReader(path));
		if (!reader->ok()) {
			return pfail(ctx, NTEDIT_E_IO, std::string("cannot open ") + path);
		}
		if (skip) {
			reader->skip(skip);
		}
		std::string blob, hdr;
		auto flush = [&]() {
			if (blob.empty()) {
				return 0;
			}
			const auto g0 = std::chrono::steady_clock::now();
			const int rc = ntedit_hip_filter_insert(ctx, slot, blob.data(), blob.size(), NTEDIT_HIP_BASES_HOST);
			gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
			blob.clear();
			return rc ? pfail(ctx, rc, std::string("filter_insert: ") + ntedit_hip_last_error(ctx)) : 0;
		};
		for (;;) {
			const size_t before = blob.size();
			if (!reader->next(hdr, blob)) {
				break;
			}
			bases += blob.size() - before;
			if (insert && blob.size() - before >= k) {
				blob.push_back('\n'); // (no k-mer spans a separator)
			} else {
				blob.resize(before);
			}
			if (blob.size() >= HOST_FLUSH) {
				const int rc = flush();
				if (rc) {
					return rc;
				}
			}
		}
		if (reader->io_error()) {
			return pfail(ctx, NTEDIT_E_IO, std::string(path) + ": " + reader->io_error_text());
		}
		return flush();
	}

	// what a parsed chunk means for its file; *unclean: hand the file back
	int chunk_done(const ntedit_hip_genome_parse_result& res, const char* batch, uint64_t n_raw, uint64_t chunk_off, uint64_t* rec_start,
	               bool* unclean)
	{
		if (!res.clean) {
			info->broken |= res.broken;
			*unclean = true;
			return 0;
		}
		const int rc = insert_batch(batch, res.text_len);
		if (rc) {
			return rc;
		}
		info->device_chunks++;
		info->raw_bytes += n_raw;
		info->text_bytes += res.text_len;
		bases += res.bases;
		if (res.last_header != NO_START) {
			*rec_start = chunk_off + res.last_header;
		}
		return 0;
	}

	// chunk i: the file's bytes [i * batch_bytes, ...), read by the feed's thread; its copy runs while the chunk before is
	// parsed and inserted
	int plain_file(const char* path, uint64_t size)
	{
		const uint64_t bases_before = bases;
		uint64_t rec_start = NO_START;
		bool unclean = false;
		int state = NTEDIT_GENOME_LINE_START;
		int rc = nte_reads::genome_begin_file(ctx);
		if (rc == 0) {
			nte_host::Feed<nte_host::RawChunk> feed(nte_host::RawProducer{ path, 0, size, (size_t)batch_bytes, nte_host::CUT_ANYWHERE });
			auto begin = [&](const nte_host::RawChunk& c, int which) { return nte_reads::parse_copy_begin(ctx, which, c.buf.p, c.len); };
			auto work = [&](const nte_host::RawChunk& c, int which, auto release) {
				const auto g0 = std::chrono::steady_clock::now();
				const char* batch = nullptr;
				ntedit_hip_genome_parse_result res = ntedit_hip_genome_parse_result();
				const uint64_t off = c.off, len = c.len;
				int rc = nte_reads::genome_parse_buffer(ctx, which, 1, len, state, off == 0, &batch, &res);
				if (rc == 0) {
					release(); // (its copy is done: the reader may fill it again)
					rc = chunk_done(res, batch, len, off, &rec_start, &unclean);
				}
				gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
				state = res.state_out;
				return rc ? rc : unclean ? (int)nte_host::OVERLAP_STOP : 0;
			};
			rc = nte_host::overlap(feed, begin, work, [&](int which) { return nte_reads::parse_copy_wait(ctx, which); });
			rc = rc == nte_host::OVERLAP_FEED ? feed_fail(ctx, feed.error()) : rc == nte_host::OVERLAP_STOP ? 0 : rc;
		}
		if (rc == 0 && unclean) {
			info->handed_back++;
			if (!insert) {
				bases = bases_before;
			}
			rc = host_parse(path, insert && rec_start != NO_START ? rec_start : 0, 0);
		}
		return rc;
	}

	// serial: a chunk is gathered, then inflated from its page-locked buffer, parsed and inserted
	int bgzf_file(const char* path)
	{
		nte_host::BgzfGather gather(path, (size_t)batch_bytes);
		if (!gather.error().empty()) {
			return pfail(ctx, NTEDIT_E_IO, gather.error());
		}
		info->bgzf_files++;
		nte_host::BgzfChunk c;
		std::vector<uint32_t> status;
		const uint64_t bases_before = bases;
		uint64_t out_off = 0;          // inflated bytes before the chunk
		uint64_t rec_start = NO_START; // an inflated offset
		bool unclean = false;
		int state = NTEDIT_GENOME_LINE_START;
		int rc = nte_reads::genome_begin_file(ctx);
		while (rc == 0 && !unclean && gather.next(&c)) {
			unclean = c.last && !c.whole; // no member starts there, or the file ends inside one: what is left is the host parser's
			if (!c.n_members) {
				break;
			}
			const auto g0 = std::chrono::steady_clock::now();
			bool bad = false; // the chunk is unclean
			if (c.n_out) {
				char* d_raw = nullptr;
				status.assign(c.n_members, 0);
				rc = nte_reads::genome_raw_buffer(ctx, 0, c.n_out, &d_raw);
				if (rc == 0) {
					rc = ntedit_hip_reads_inflate_device(ctx, c.buf.p, c.len, NTEDIT_HIP_BASES_HOST, c.m(), c.n_members, d_raw, c.n_out,
					                                     status.data());
				}
				for (size_t m = 0; rc == 0 && m < c.n_members; m++) {
					if (status[m]) {
						rc = pfail(ctx, NTEDIT_E_IO, std::string(path) + ": BGZF member " + std::to_string(c.first_member + m) +
						                                 " is damaged (" + nte_reads::inflate_reason(status[m]) + ")");
					}
				}
				const char* batch = nullptr;
				ntedit_hip_genome_parse_result res = ntedit_hip_genome_parse_result();
				if (rc == 0) {
					rc = nte_reads::genome_parse_buffer(ctx, 0, 0, c.n_out, state, out_off == 0, &batch, &res);
				}
				if (rc == 0) {
					rc = chunk_done(res, batch, c.n_out, out_off, &rec_start, &bad);
					state = res.state_out;
				}
			}
			if (bad) {
				unclean = true;
			} else if (rc == 0) {
				info->bgzf_members += c.n_members; // (the empty member at the file's end included)
			}
			gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
			out_off += c.n_out;
		}
		if (rc == 0 && !gather.error().empty()) {
			rc = feed_fail(ctx, gather.error());
		}
		if (rc == 0 && unclean) {
			info->handed_back++;
			if (!insert) {
				bases = bases_before;
			}
			rc = host_parse(path, 0, insert && rec_start != NO_START ? rec_start : 0);
		}
		return rc;
	}
};

} // namespace

extern "C" {

int
ntedit_hip_genome_pass(ntedit_hip_ctx* ctx, int slot, const char* const* files, uint32_t n, uint64_t batch_bytes, int insert,
                       ntedit_hip_reads_pass_stats* stats)
{
	if (!ctx || (n && !files)) {
		return pfail(ctx, NTEDIT_E_ARG, "genome_pass: bad argument");
	}
	Pass p;
	p.ctx = ctx;
	p.slot = slot;
	p.insert = insert ? 1 : 0;
	p.batch_bytes = batch_bytes < nte_host::CHUNK_MAX ? batch_bytes : nte_host::CHUNK_MAX;
	p.info = nte_reads::genome_info(ctx);
	*p.info = ntedit_hip_genome_pass_info();
	if (insert) {
		uint32_t hash_num = 0;
		uint64_t nbytes = 0;
		int counting = 0;
		if (ntedit_hip_filter_info(ctx, slot, &p.k, &hash_num, &nbytes, &counting) != 0 || p.k < 2 ||
		    p.k > (uint32_t)nte_reads::genome_pad()) {
			return pfail(ctx, NTEDIT_E_ARG, "genome_pass: no filter in the slot (ntedit_hip_filter_alloc), or a k the carried text cannot hold");
		}
	}
	const auto t0 = std::chrono::steady_clock::now();
	for (uint32_t i = 0; i < n; i++) {
		struct stat sb;
		if (!files[i] || stat(files[i], &sb) != 0) {
			return pfail(ctx, NTEDIT_E_IO, std::string("cannot open ") + (files[i] ? files[i] : "(null)"));
		}
		int first = -1;
		const int kind = S_ISREG(sb.st_mode) ? nte_host::file_kind(files[i], &first) : 1;
		int rc;
		if (kind == 2 && batch_bytes) {
			rc = p.bgzf_file(files[i]);
		} else if (batch_bytes == 0 || kind == 1 || first != '>') {
			p.info->host_files++;
			rc = p.host_parse(files[i], 0, 0);
		} else {
			rc = p.plain_file(files[i], (uint64_t)sb.st_size);
		}
		if (rc) {
			return rc;
		}
	}
	if (stats) {
		stats->bases = p.bases;
		stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		stats->ms_gpu = p.gpu_ms;
	}
	return 0;
}

int
ntedit_hip_genome_pass_line(ntedit_hip_ctx* ctx, char* out, uint64_t cap)
{
	ntedit_hip_genome_pass_info gi;
	if (!out || cap == 0 || ntedit_hip_genome_pass_get_info(ctx, &gi) != 0) {
		return NTEDIT_E_ARG;
	}
	char ms[64];
	snprintf(ms, sizeof ms, "%.1f", gi.ms_kernels);
	std::string l = "--gpu_parse: genome: " + std::to_string(gi.device_chunks) + " chunks parsed on the device (" +
	                std::to_string(gi.raw_bytes) + " raw bytes, " + std::to_string(gi.text_bytes) + " text bytes, " + ms +
	                " ms in the parse kernels), " + std::to_string(gi.handed_back) + (gi.handed_back == 1 ? " file" : " files") +
	                " handed back";
	if (gi.handed_back) {
		static const char* const rules[] = { "the first byte is not '>'", "a carriage return", "an empty line",
			                                 "a sequence line that starts with '+' or '@'", "", "", "", "",
			                                 "more than one line per 8 bytes", "a chunk of 2 GiB or more" };
		std::string whys;
		for (int b = 0; b < 10; b++) {
			if ((gi.broken & (1u << b)) && rules[b][0]) {
				whys += (whys.empty() ? "" : "; ") + std::string(rules[b]);
			}
		}
		l += " to the host parser (" + (whys.empty() ? std::string("what follows the BGZF members is not BGZF") : whys) + ")";
	}
	l += "; " + std::to_string(gi.host_files) + (gi.host_files == 1 ? " file" : " files") + " left to the host parser";
	if (gi.bgzf_files) {
		l += "; BGZF: " + std::to_string(gi.bgzf_members) + " members of " + std::to_string(gi.bgzf_files) +
		     (gi.bgzf_files == 1 ? " file" : " files") + " inflated on the device";
	}
	snprintf(out, (size_t)cap, "%s", l.c_str());
	return 0;
}

} // extern "C"
