// genome_pass.cpp -- the host side of --gpu_parse for genome FASTA, shared by ntedit-make-genome-bf and ntedit --genome:
// one pass over the genome files that either inserts every k-mer into a filter slot or only adds up the bases (the
// sizing pass).  A file goes to the device in chunks of batch_bytes raw bytes cut wherever they end -- a chromosome is
// longer than any chunk -- and the stateful grammar (nte_genome_grammar.h) carries what a cut hides: each chunk is
// entered in its predecessor's exit state.  The chunk's text lands behind the last k - 1 text bytes of its file, so the
// k-mers across a cut are in the batch that ntedit_hip_filter_insert gets; insertion is idempotent, so the overlap
// changes no bit.
//
//   plain files   pread into two page-locked buffers and copied on the copy stream by a reader thread while the chunk
//                 before is parsed and inserted
//   BGZF files    shipped compressed, in whole members whose ISIZE sum stays within batch_bytes, and inflated on the
//                 device (ntedit_hip_reads_inflate_device); no cut is looked for, the state carries over
//   hand-back     from the first unclean chunk of a file on the host parser takes the file, from the last record start
//                 known from the clean chunks before it (their last_header), or from offset 0; the sizing pass reads
//                 such a file again from its start, so that no base is counted twice
//   host files    single-stream .gz files and files that do not start with '>' take the host parser whole, and with
//                 batch_bytes 0 every file does (the pass without --gpu_parse)
#include "../../include/ntedit_hip.h"
#include "fasta.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace nte_reads {
int set_error(const ntedit_hip_ctx* c, int code, const std::string& why);
const char* inflate_reason(uint32_t st);
int parse_copy_begin(const ntedit_hip_ctx* c, int which, const char* host, uint64_t n);
int parse_copy_wait(const ntedit_hip_ctx* c, int which);
// the genome chunks of nte_reads_parse.hip
ntedit_hip_genome_pass_info* genome_info(const ntedit_hip_ctx* c);
int genome_pad(void);
int genome_begin_file(const ntedit_hip_ctx* c);
int genome_raw_buffer(const ntedit_hip_ctx* c, int which, uint64_t n, char** d_raw);
int genome_parse_buffer(const ntedit_hip_ctx* c, int which, int copied, uint64_t n, int state_in, int first_chunk, const char** batch,
                        ntedit_hip_genome_parse_result* res);
int genome_carry(const ntedit_hip_ctx* c, uint64_t text_len, uint32_t keep);
}

namespace {

const uint64_t NO_START = NTEDIT_READS_NO_START;
const uint64_t CHUNK_MAX = 1u << 30;    // (the device parser takes chunks below 2^31 bytes)
const size_t HOST_FLUSH = 512u << 20;   // the host parser's batches, as ntedit-make-genome-bf makes them

int
pfail(const ntedit_hip_ctx* c, int code, const std::string& why)
{
	return nte_reads::set_error(c, code, why);
}

bool
pread_whole(int fd, char* p, uint64_t off, size_t n)
{
	while (n) {
		const ssize_t got = pread(fd, p, n, (off_t)off);
		if (got <= 0) {
			return false;
		}
		p += got, off += (uint64_t)got, n -= (size_t)got;
	}
	return true;
}

struct Pinned
{
	char* p = nullptr;
	size_t cap = 0;
	~Pinned() { ntedit_hip_host_free(p); }
	bool reserve(size_t need, size_t keep)
	{
		if (need <= cap) {
			return true;
		}
		char* q = (char*)ntedit_hip_host_alloc(need);
		if (!q) {
			return false;
		}
		if (keep) {
			memcpy(q, p, keep);
		}
		ntedit_hip_host_free(p);
		p = q;
		cap = need;
		return true;
	}
};

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

	int plain_file(const char* path, uint64_t size)
	{
		const int fd = open(path, O_RDONLY);
		if (fd < 0) {
			return pfail(ctx, NTEDIT_E_IO, std::string("cannot open ") + path);
		}
		Pinned buf[2];
		const uint64_t bases_before = bases;
		uint64_t rec_start = NO_START;
		bool unclean = false;
		int rc = nte_reads::genome_begin_file(ctx);
		// chunk i: bytes [i * batch, ...) through buffer i & 1; read and queued for its copy by this
		auto feed = [&](uint64_t off, int which) -> int {
			const size_t len = (size_t)(size - off < batch_bytes ? size - off : batch_bytes);
			if (!buf[which].reserve(len, 0)) {
				return pfail(ctx, NTEDIT_E_DEVICE, "cannot allocate page-locked host memory");
			}
			if (!pread_whole(fd, buf[which].p, off, len)) {
				return pfail(ctx, NTEDIT_E_IO, std::string(path) + ": read error");
			}
			return nte_reads::parse_copy_begin(ctx, which, buf[which].p, len);
		};
		if (rc == 0) {
			rc = feed(0, 0);
		}
		int state = NTEDIT_GENOME_LINE_START, which = 0;
		for (uint64_t off = 0; rc == 0 && off < size && !unclean; off += batch_bytes, which ^= 1) {
			const uint64_t len = size - off < batch_bytes ? size - off : batch_bytes;
			// chunk i + 1 is read and copied while chunk i is parsed and inserted
			std::future<int> next;
			if (off + batch_bytes < size) {
				next = std::async(std::launch::async, feed, off + batch_bytes, which ^ 1);
			}
			const auto g0 = std::chrono::steady_clock::now();
			const char* batch = nullptr;
			ntedit_hip_genome_parse_result res = ntedit_hip_genome_parse_result();
			rc = nte_reads::genome_parse_buffer(ctx, which, 1, len, state, off == 0, &batch, &res);
			if (rc == 0) {
				rc = chunk_done(res, batch, len, off, &rec_start, &unclean);
			}
			gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
			state = res.state_out;
			if (next.valid()) {
				const int rc_next = next.get();
				(void)nte_reads::parse_copy_wait(ctx, which ^ 1); // (before the buffer it reads may go)
				rc = rc ? rc : rc_next;
			}
		}
		close(fd);
		if (rc == 0 && unclean) {
			info->handed_back++;
			if (!insert) {
				bases = bases_before;
			}
			rc = host_parse(path, insert && rec_start != NO_START ? rec_start : 0, 0);
		}
		return rc;
	}

	int bgzf_file(const char* path, uint64_t size)
	{
		const int fd = open(path, O_RDONLY);
		if (fd < 0) {
			return pfail(ctx, NTEDIT_E_IO, std::string("cannot open ") + path);
		}
		info->bgzf_files++;
		Pinned comp;
		std::vector<ntedit_hip_bgzf_member> members;
		std::vector<uint32_t> status;
		const size_t slab = (size_t)(batch_bytes / 4 + (128u << 10)); // compressed bytes read at a time
		const uint64_t bases_before = bases;
		uint64_t pos = 0, have = 0;     // comp holds the file's bytes [pos, pos + have)
		uint64_t out_off = 0;           // inflated bytes before the chunk
		uint64_t rec_start = NO_START;  // an inflated offset
		uint64_t first_member = 0;
		bool unclean = false, done = false;
		int state = NTEDIT_GENOME_LINE_START;
		int rc = nte_reads::genome_begin_file(ctx);
		while (rc == 0 && !done && !unclean) {
			// whole members whose ISIZE sum stays within batch_bytes (at least one)
			members.clear();
			uint64_t walked = 0, n_out = 0;
			for (;;) {
				ntedit_hip_bgzf_member one;
				uint64_t found = 0, used = 0;
				const int why = ntedit_hip_bgzf_walk(comp.p + walked, have - walked, &one, 1, &found, &used);
				if (found) {
					if (!members.empty() && n_out + one.n_out > batch_bytes) {
						break;
					}
					one.in_off += walked;
					one.out_off = n_out;
					members.push_back(one);
					n_out += one.n_out;
					walked += used;
					continue;
				}
				if (why == NTEDIT_BGZF_NOT || pos + have >= size) {
					// no member starts here, or the file ends inside one: what is left is the host parser's
					done = true;
					unclean = have != walked;
					break;
				}
				const size_t more = (size_t)(size - (pos + have) < slab ? size - (pos + have) : slab);
				if (!comp.reserve((size_t)have + more, (size_t)have)) {
					rc = pfail(ctx, NTEDIT_E_DEVICE, "cannot allocate page-locked host memory");
					break;
				}
				if (!pread_whole(fd, comp.p + have, pos + have, more)) {
					rc = pfail(ctx, NTEDIT_E_IO, std::string(path) + ": read error");
					break;
				}
				have += more;
			}
			if (rc || members.empty()) {
				break;
			}
			const auto g0 = std::chrono::steady_clock::now();
			bool bad = false; // the chunk is unclean
			if (n_out) {
				char* d_raw = nullptr;
				status.assign(members.size(), 0);
				rc = nte_reads::genome_raw_buffer(ctx, 0, n_out, &d_raw);
				if (rc == 0) {
					rc = ntedit_hip_reads_inflate_device(ctx, comp.p, walked, NTEDIT_HIP_BASES_HOST, members.data(), members.size(), d_raw,
					                                     n_out, status.data());
				}
				for (size_t m = 0; rc == 0 && m < members.size(); m++) {
					if (status[m]) {
						rc = pfail(ctx, NTEDIT_E_IO, std::string(path) + ": BGZF member " + std::to_string(first_member + m) +
						                                 " is damaged (" + nte_reads::inflate_reason(status[m]) + ")");
					}
				}
				const char* batch = nullptr;
				ntedit_hip_genome_parse_result res = ntedit_hip_genome_parse_result();
				if (rc == 0) {
					rc = nte_reads::genome_parse_buffer(ctx, 0, 0, n_out, state, out_off == 0, &batch, &res);
				}
				if (rc == 0) {
					rc = chunk_done(res, batch, n_out, out_off, &rec_start, &bad);
					state = res.state_out;
				}
			}
			if (bad) {
				unclean = true;
				done = true;
			} else if (rc == 0) {
				info->bgzf_members += members.size(); // (the empty member at the file's end included)
			}
			gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
			out_off += n_out;
			first_member += members.size();
			if (have > walked) {
				memmove(comp.p, comp.p + walked, (size_t)(have - walked));
			}
			pos += walked;
			have -= walked;
		}
		close(fd);
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

// 0: plain, 1: a single-stream gzip file, 2: BGZF; *first: the file's first byte (-1: empty or unreadable)
int
file_kind(const char* path, int* first)
{
	unsigned char head[4096];
	FILE* fp = fopen(path, "rb");
	const size_t got = fp ? fread(head, 1, sizeof head, fp) : 0;
	if (fp) {
		fclose(fp);
	}
	*first = got ? (int)head[0] : -1;
	if (got < 2 || head[0] != 0x1f || head[1] != 0x8b) {
		return 0;
	}
	uint64_t found = 0, used = 0;
	const int why = ntedit_hip_bgzf_walk(head, got, nullptr, 0, &found, &used);
	return got >= 28 && (why == NTEDIT_BGZF_FULL || (why == NTEDIT_BGZF_CUT && got == sizeof head)) ? 2 : 1;
}

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
	p.batch_bytes = batch_bytes < CHUNK_MAX ? batch_bytes : CHUNK_MAX;
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
		const int kind = S_ISREG(sb.st_mode) ? file_kind(files[i], &first) : 1;
		int rc;
		if (kind == 2 && batch_bytes) {
			rc = p.bgzf_file(files[i], (uint64_t)sb.st_size);
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
