// reads_pass.cpp -- the host side of the reads k-mer filter build, shared by ntedit-make-reads-bf and the sharded driver
// (ntedit_amd/make_reads.py): one pass over a list of byte ranges of the input files, parsed by FastaReader into bounded
// batches double-buffered through page-locked memory (a second thread parses the next batch while the GPU works on the
// current one); the tool's sizing; its --hist writer; and the build itself, in four stages that both walk.  With a reject
// cutoff the build's pass 2 fills the SECONDARY slot too (the filter ntedit -e loads), from the same walk.
//
// A range [begin, end) of a file owns the records whose first byte lies in it.  A range that starts past byte 0 first
// moves forward to the first record start: a line that starts with '>' in a FASTA file, or in a FASTQ file a line that
// starts with '@' whose line + 2 starts with '+' (unambiguous for 4-line FASTQ).  The parser then runs with kseq's rules
// and stops before the first record that starts at or past `end`; where it stopped is reported (`nexts`), as is where
// the range started (`starts`).  Only when every range's stop is the next range's start did the ranges parse the file
// exactly as one reader would: the driver checks that after pass 1 (multi-line FASTQ can break it).  Gzip files are
// single units.
#include "../../include/ntedit_hip.h"
#include "fasta.h"

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace nte_reads {
int set_error(const ntedit_hip_ctx* c, int code, const std::string& why);
uint32_t reject_cutoff(const ntedit_hip_ctx* c); // ntedit_hip_reads_set_reject_cutoff (nte_reads.hip)
uint32_t min_read(const ntedit_hip_ctx* c, uint32_t k); // ntedit_hip_reads_set_min_read: the shortest record kept, k at most
// --gpu_parse (nte_reads_parse.hip): the context's setting and counters, its two raw buffers and its copy stream
int parse_is_on(const ntedit_hip_ctx* c);
ntedit_hip_reads_parse_stats* parse_info(const ntedit_hip_ctx* c);
int parse_copy_begin(const ntedit_hip_ctx* c, int which, const char* host, uint64_t n);
int parse_copy_wait(const ntedit_hip_ctx* c, int which);
int parse_copied(const ntedit_hip_ctx* c, int which, uint64_t n, uint32_t k, const char** text, ntedit_hip_reads_parse_result* res);
int parse_buffer(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, uint32_t k, const char** text, ntedit_hip_reads_parse_result* res);
// --gpu_parse on BGZF files (nte_reads_inflate.hip): its counters, its two compressed buffers, the inflated chunk
ntedit_hip_reads_inflate_stats* inflate_info(const ntedit_hip_ctx* c);
const char* inflate_reason(uint32_t st);
int inflate_copy_begin(const ntedit_hip_ctx* c, int which, const char* comp, uint64_t n_comp, const ntedit_hip_bgzf_member* members,
                       uint64_t n_members);
int inflate_copy_wait(const ntedit_hip_ctx* c, int which);
int inflate_copied(const ntedit_hip_ctx* c, int which, uint64_t n_comp, const ntedit_hip_bgzf_member* members, uint64_t n_members,
                   uint64_t tail, uint64_t n_out, const char** raw, uint64_t* bad, uint32_t* reason);
int inflate_last_start(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, uint64_t* cut, uint32_t* broken);
int inflate_carry(const ntedit_hip_ctx* c, uint64_t cut, uint64_t total);
// ... and on BAM files (nte_reads_bam.hip): its counters, and the walk and decode of an inflated chunk
ntedit_hip_reads_bam_stats* bam_info(const ntedit_hip_ctx* c);
int bam_buffer(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, int at_header, uint32_t min_len, const char** text,
               ntedit_hip_reads_bam_result* res);
}

namespace {

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

bool
is_gzip(const char* path)
{
	unsigned char magic[2] = { 0, 0 };
	FILE* fp = fopen(path, "rb");
	const bool gz = fp && fread(magic, 1, 2, fp) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
	if (fp) {
		fclose(fp);
	}
	return gz;
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

// every record of one range, in order: seq(record) for each; *start / *next as ntedit_hip_reads_pass reports them
bool
read_range(const char* path, uint64_t begin, uint64_t end, const std::function<bool(const std::string&)>& seq_fn,
           uint64_t* start, uint64_t* next, std::string* why, bool exact = false, uint64_t skip = 0)
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
	std::string hdr, seq;
	for (;;) {
		seq.clear();
		if (!reader.next(hdr, seq)) {
			break;
		}
		if (!seq_fn(seq)) {
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

// page-locked batch buffers: the parser fills one while the GPU works on the other
struct Batch
{
	char* p = nullptr;
	size_t cap = 0, len = 0;
	uint64_t bases = 0;
	bool last = false;
};

class BatchFeeder
{
  public:
	BatchFeeder(const std::vector<Range>& ranges, unsigned k, size_t batch_bytes, uint64_t* starts, uint64_t* nexts)
	    : ranges_(ranges), k_(k), batch_bytes_(batch_bytes), starts_(starts), nexts_(nexts)
	{
		for (Batch& b : bufs_) {
			free_.push_back(&b);
		}
		th_ = std::thread([this] { run_(); });
	}
	~BatchFeeder()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		th_.join();
		for (Batch& b : bufs_) {
			ntedit_hip_host_free(b.p);
		}
	}
	// the next filled batch (last = true: the input ends with it); nullptr after an error
	Batch* take()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [this] { return !full_.empty() || failed_; });
		if (failed_) {
			return nullptr;
		}
		Batch* b = full_.front();
		full_.pop_front();
		return b;
	}
	void give_back(Batch* b)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			free_.push_back(b);
		}
		cv_.notify_all();
	}
	const std::string& error() const { return err_; }

  private:
	Batch* get_free_()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [this] { return !free_.empty() || stop_; });
		if (stop_) {
			return nullptr;
		}
		Batch* b = free_.front();
		free_.pop_front();
		b->len = 0;
		b->bases = 0;
		b->last = false;
		return b;
	}
	void put_full_(Batch* b)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			full_.push_back(b);
		}
		cv_.notify_all();
	}
	void fail_(const std::string& why)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			err_ = why;
			failed_ = true;
		}
		cv_.notify_all();
	}
	bool reserve_(Batch* b, size_t need)
	{
		if (need <= b->cap) {
			return true;
		}
		const size_t cap = need > batch_bytes_ ? need : batch_bytes_;
		char* p = (char*)ntedit_hip_host_alloc(cap);
		if (!p) {
			return false;
		}
		if (b->len) {
			memcpy(p, b->p, b->len);
		}
		ntedit_hip_host_free(b->p);
		b->p = p;
		b->cap = cap;
		return true;
	}
	// one read into the batch; false: stop (stopped, or failed)
	bool add_(Batch*& b, const std::string& seq)
	{
		if (seq.size() < k_) { // no k-mer in it
			return true;
		}
		// reads are separated by '\n' (no k-mer spans a separator)
		if (b->len && b->len + seq.size() + 1 > batch_bytes_) {
			put_full_(b);
			if (!(b = get_free_())) {
				return false;
			}
		}
		if (!reserve_(b, b->len + seq.size() + 1)) {
			fail_("cannot allocate page-locked host memory");
			return false;
		}
		memcpy(b->p + b->len, seq.data(), seq.size());
		b->p[b->len + seq.size()] = '\n';
		b->len += seq.size() + 1;
		b->bases += seq.size();
		return true;
	}
	void run_()
	{
		Batch* b = get_free_();
		for (size_t i = 0; i < ranges_.size(); i++) {
			if (!b) {
				return;
			}
			const Range& r = ranges_[i];
			uint64_t start = 0, next = 0;
			bool stopped = false;
			std::string why;
			auto add = [&](const std::string& seq) {
				stopped = !add_(b, seq);
				return !stopped;
			};
			const bool ok = read_range(r.path, r.begin, r.end, add, &start, &next, &why, r.exact, r.skip);
			if (stopped) {
				return; // (add_ failed the feeder, or it is being torn down)
			}
			if (!ok) {
				fail_(why);
				return;
			}
			if (starts_) {
				starts_[i] = start;
			}
			if (nexts_) {
				nexts_[i] = next;
			}
		}
		if (b) {
			b->last = true;
			put_full_(b);
		}
	}

	std::vector<Range> ranges_;
	unsigned k_;
	size_t batch_bytes_;
	uint64_t *starts_, *nexts_;
	Batch bufs_[2];
	std::deque<Batch*> free_, full_;
	bool stop_ = false, failed_ = false;
	std::string err_;
	std::mutex mu_;
	std::condition_variable cv_;
	std::thread th_;
};


// ------------------------------------------------------------------ --gpu_parse: raw chunks instead of parsed batches
const size_t NONE = ~(size_t)0;
const size_t RAW_CHUNK_MAX = 1u << 30; // (the device parser takes chunks below 2^31 bytes)
const unsigned RAW_READERS = 4;        // threads that pread slices of one chunk
const size_t RAW_SLICE_MIN = 4u << 20;

// the last record start in buf(0, n) by find_record_start's rule for a chunk of this kind: '>' at a line start, or an
// '@' line whose line + 2 (inside the buffer) starts with '+'; NONE when there is none
size_t
last_record_start(const char* buf, size_t n, int kind)
{
	if (kind == '>') {
		for (size_t end = n; end > 1;) {
			const char* q = (const char*)memrchr(buf + 1, '>', end - 1);
			if (!q) {
				break;
			}
			if (q[-1] == '\n') {
				return (size_t)(q - buf);
			}
			end = (size_t)(q - buf);
		}
		return NONE;
	}
	size_t l1 = NONE, l2 = NONE; // the starts of the two lines behind the current one
	for (size_t end = n; end >= 2;) {
		const char* q = (const char*)memrchr(buf, '\n', end - 1);
		if (!q) {
			break;
		}
		const size_t cur = (size_t)(q - buf) + 1;
		if (l2 != NONE && buf[cur] == '@' && buf[l2] == '+') {
			return cur;
		}
		l2 = l1;
		l1 = cur;
		end = cur;
	}
	return NONE;
}

// file bytes [off, off + n) into p, by a few threads: raw reading has no order
bool
pread_all(int fd, char* p, uint64_t off, size_t n)
{
	auto slice = [fd](char* q, uint64_t at, size_t len) {
		while (len) {
			const ssize_t got = pread(fd, q, len, (off_t)at);
			if (got <= 0) {
				return false;
			}
			q += got, at += (uint64_t)got, len -= (size_t)got;
		}
		return true;
	};
	const size_t parts = n / RAW_SLICE_MIN < RAW_READERS ? (n / RAW_SLICE_MIN ? n / RAW_SLICE_MIN : 1) : RAW_READERS;
	if (parts == 1) {
		return slice(p, off, n);
	}
	std::vector<std::thread> th;
	std::vector<char> ok(parts, 0);
	for (size_t i = 0; i < parts; i++) {
		const size_t a = n * i / parts, b = n * (i + 1) / parts;
		th.emplace_back([&, i, a, b] { ok[i] = slice(p + a, off + a, b - a); });
	}
	bool all = true;
	for (size_t i = 0; i < parts; i++) {
		th[i].join();
		all = all && ok[i];
	}
	return all;
}

// The bytes [start, stop) of one plain file (start a record start, stop a record start or the file's end) as chunks of
// about batch_bytes raw bytes, each cut at its last record start, the tail carried into the next; double-buffered through
// page-locked memory as BatchFeeder's batches are.  A chunk without a record start past its first byte grows by another
// batch_bytes (a record longer than a batch).
struct RawChunk
{
	char* p = nullptr;
	size_t cap = 0, len = 0;
	uint64_t off = 0; // of its first byte in the file
	bool last = false;
};

class RawFeeder
{
  public:
	RawFeeder(const char* path, uint64_t start, uint64_t stop, size_t batch_bytes)
	    : path_(path), pos_(start), stop_at_(stop), batch_bytes_(batch_bytes < RAW_CHUNK_MAX ? batch_bytes : RAW_CHUNK_MAX)
	{
		for (RawChunk& b : bufs_) {
			free_.push_back(&b);
		}
		th_ = std::thread([this] { run_(); });
	}
	~RawFeeder()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		th_.join();
		for (RawChunk& b : bufs_) {
			ntedit_hip_host_free(b.p);
		}
	}
	RawChunk* take()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [this] { return !full_.empty() || failed_; });
		if (full_.empty()) {
			return nullptr;
		}
		RawChunk* b = full_.front();
		full_.pop_front();
		return b;
	}
	void give_back(RawChunk* b)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			free_.push_back(b);
		}
		cv_.notify_all();
	}
	const std::string& error() const { return err_; }

  private:
	void fail_(const std::string& why)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			err_ = why;
			failed_ = true;
		}
		cv_.notify_all();
	}
	bool reserve_(RawChunk* b, size_t need, size_t keep)
	{
		if (need <= b->cap) {
			return true;
		}
		char* p = (char*)ntedit_hip_host_alloc(need);
		if (!p) {
			return false;
		}
		if (keep) {
			memcpy(p, b->p, keep);
		}
		ntedit_hip_host_free(b->p);
		b->p = p;
		b->cap = need;
		return true;
	}
	void run_()
	{
		const int fd = open(path_, O_RDONLY);
		if (fd < 0) {
			fail_(std::string("cannot open ") + path_);
			return;
		}
		std::vector<char> tail;
		while (pos_ < stop_at_) {
			RawChunk* b;
			{
				std::unique_lock<std::mutex> lk(mu_);
				cv_.wait(lk, [this] { return !free_.empty() || stop_; });
				if (stop_) {
					break;
				}
				b = free_.front();
				free_.pop_front();
			}
			size_t have = tail.size(), want = batch_bytes_ > have ? batch_bytes_ : have + batch_bytes_;
			bool ok = reserve_(b, want, 0);
			if (ok && have) {
				memcpy(b->p, tail.data(), have);
			}
			size_t cut = NONE;
			while (ok) {
				if ((uint64_t)want > stop_at_ - pos_) {
					want = (size_t)(stop_at_ - pos_);
				}
				if (!pread_all(fd, b->p + have, pos_ + have, want - have)) {
					fail_(std::string(path_) + ": read error");
					close(fd);
					return;
				}
				have = want;
				if (pos_ + have == stop_at_) {
					cut = have; // the range's last chunk ends where the range does
					break;
				}
				const int kind = (unsigned char)b->p[0];
				cut = kind == '>' || kind == '@' ? last_record_start(b->p, have, kind) : have; // (neither: unclean anyway)
				if (cut != NONE) {
					break;
				}
				want = have + batch_bytes_;
				ok = reserve_(b, want, have);
			}
			if (!ok) {
				fail_("cannot allocate page-locked host memory");
				close(fd);
				return;
			}
			tail.assign(b->p + cut, b->p + have);
			b->len = cut;
			b->off = pos_;
			pos_ += cut;
			b->last = pos_ >= stop_at_;
			{
				std::lock_guard<std::mutex> lk(mu_);
				full_.push_back(b);
			}
			cv_.notify_all();
		}
		close(fd);
	}

	const char* path_;
	uint64_t pos_, stop_at_;
	size_t batch_bytes_;
	RawChunk bufs_[2];
	std::deque<RawChunk*> free_, full_;
	bool stop_ = false, failed_ = false;
	std::string err_;
	std::mutex mu_;
	std::condition_variable cv_;
	std::thread th_;
};

// ------------------------------------------------------------------ --gpu_parse: BGZF files stay compressed
// Whether the file starts with a BGZF member (bgzf_walk finds one, or finds its header and the buffer's end)
bool
is_bgzf(const char* path)
{
	unsigned char head[4096];
	FILE* fp = fopen(path, "rb");
	const size_t got = fp ? fread(head, 1, sizeof head, fp) : 0;
	if (fp) {
		fclose(fp);
	}
	uint64_t found = 0, used = 0;
	const int rc = ntedit_hip_bgzf_walk(head, got, nullptr, 0, &found, &used);
	return got >= 28 && (rc == NTEDIT_BGZF_FULL || (rc == NTEDIT_BGZF_CUT && got == sizeof head));
}

// A BGZF file as chunks of whole members whose ISIZE sum stays within batch_bytes (at least one member), compressed,
// double-buffered through page-locked memory as RawFeeder's chunks are; nothing is inflated here.  The last chunk says
// how the members ended: with the file, or at something that is no (whole) BGZF member.
struct BgzfChunk
{
	char* p = nullptr;
	size_t cap = 0, len = 0; // len: the compressed bytes of its members
	ntedit_hip_bgzf_member* m = nullptr;
	size_t m_cap = 0, n_members = 0;
	uint64_t n_out = 0;        // their ISIZE sum
	uint64_t first_member = 0; // the index of m[0] in the file
	bool last = false;
	bool whole = true; // (last) the file ended behind a whole member
};

class BgzfFeeder
{
  public:
	BgzfFeeder(const char* path, size_t batch_bytes)
	    : path_(path), batch_bytes_(batch_bytes < RAW_CHUNK_MAX ? batch_bytes : RAW_CHUNK_MAX)
	{
		for (BgzfChunk& b : bufs_) {
			free_.push_back(&b);
		}
		th_ = std::thread([this] { run_(); });
	}
	~BgzfFeeder()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		th_.join();
		for (BgzfChunk& b : bufs_) {
			ntedit_hip_host_free(b.p);
			ntedit_hip_host_free(b.m);
		}
	}
	BgzfChunk* take()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [this] { return !full_.empty() || failed_; });
		if (full_.empty()) {
			return nullptr;
		}
		BgzfChunk* b = full_.front();
		full_.pop_front();
		return b;
	}
	void give_back(BgzfChunk* b)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			free_.push_back(b);
		}
		cv_.notify_all();
	}
	const std::string& error() const { return err_; }

  private:
	void fail_(const std::string& why)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			err_ = why;
			failed_ = true;
		}
		cv_.notify_all();
	}
	static bool reserve_(char** p, size_t* cap, size_t need, size_t keep)
	{
		if (need <= *cap) {
			return true;
		}
		const size_t want = need + need / 2;
		char* q = (char*)ntedit_hip_host_alloc(want);
		if (!q) {
			return false;
		}
		if (keep) {
			memcpy(q, *p, keep);
		}
		ntedit_hip_host_free(*p);
		*p = q;
		*cap = want;
		return true;
	}
	void run_()
	{
		const int fd = open(path_, O_RDONLY);
		struct stat sb;
		if (fd < 0 || fstat(fd, &sb) != 0) {
			if (fd >= 0) {
				close(fd);
			}
			fail_(std::string("cannot open ") + path_);
			return;
		}
		const uint64_t size = (uint64_t)sb.st_size;
		const size_t slab = batch_bytes_ / 4 + (128u << 10); // compressed bytes read at a time
		std::vector<char> carry;                              // compressed bytes read behind the last chunk's members
		uint64_t pos = 0, member = 0;
		for (bool done = false; !done;) {
			BgzfChunk* b;
			{
				std::unique_lock<std::mutex> lk(mu_);
				cv_.wait(lk, [this] { return !free_.empty() || stop_; });
				if (stop_) {
					break;
				}
				b = free_.front();
				free_.pop_front();
			}
			size_t have = carry.size(), walked = 0;
			bool ok = reserve_(&b->p, &b->cap, have > slab ? have : slab, 0);
			if (ok && have) {
				memcpy(b->p, carry.data(), have);
			}
			b->n_members = 0;
			b->n_out = 0;
			b->first_member = member;
			b->last = false;
			b->whole = true;
			while (ok) {
				ntedit_hip_bgzf_member one;
				uint64_t found = 0, used = 0;
				const int rc = ntedit_hip_bgzf_walk(b->p + walked, have - walked, &one, 1, &found, &used);
				if (found) {
					if (b->n_members && b->n_out + one.n_out > batch_bytes_) {
						break; // the chunk is full
					}
					size_t m_bytes = b->m_cap * sizeof one;
					if (!(ok = reserve_((char**)&b->m, &m_bytes, (b->n_members + 1) * sizeof one, b->n_members * sizeof one))) {
						break;
					}
					b->m_cap = m_bytes / sizeof one;
					one.in_off += walked;
					one.out_off = b->n_out;
					b->m[b->n_members++] = one;
					b->n_out += one.n_out;
					walked += (size_t)used;
					continue;
				}
				if (rc == NTEDIT_BGZF_NOT || pos + have >= size) {
					// no member starts here, or the file ends inside one
					b->last = true;
					b->whole = rc != NTEDIT_BGZF_NOT && have == walked;
					break;
				}
				const size_t more = size - (pos + have) < slab ? (size_t)(size - (pos + have)) : slab;
				if (!(ok = reserve_(&b->p, &b->cap, have + more, have))) {
					break;
				}
				if (!pread_all(fd, b->p + have, pos + have, more)) {
					fail_(std::string(path_) + ": read error");
					close(fd);
					return;
				}
				have += more;
			}
			if (!ok) {
				fail_("cannot allocate page-locked host memory");
				close(fd);
				return;
			}
			carry.assign(b->p + walked, b->p + have);
			b->len = walked;
			pos += walked;
			member += b->n_members;
			done = b->last;
			{
				std::lock_guard<std::mutex> lk(mu_);
				full_.push_back(b);
			}
			cv_.notify_all();
		}
		close(fd);
	}

	const char* path_;
	size_t batch_bytes_;
	BgzfChunk bufs_[2];
	std::deque<BgzfChunk*> free_, full_;
	bool stop_ = false, failed_ = false;
	std::string err_;
	std::mutex mu_;
	std::condition_variable cv_;
	std::thread th_;
};

} // namespace

extern "C" {

uint64_t
ntedit_hip_reads_last_record_start(const char* buf, uint64_t n, int kind)
{
	const size_t at = buf ? last_record_start(buf, (size_t)n, kind) : NONE;
	return at == NONE ? NTEDIT_READS_NO_START : (uint64_t)at;
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
	// the shortest record the parsers keep: the sketch's k, or below it what ntedit_hip_reads_set_min_read asks for
	const uint32_t keep = nte_reads::min_read(ctx, k);
	const auto t0 = std::chrono::steady_clock::now();
	uint64_t bases = 0;
	double gpu_ms = 0.0;
	// one batch of text, host or device, through the pass's kernels (SOLID with a reject cutoff set: both slots)
	const uint32_t rmin = pass == NTEDIT_READS_PASS_SOLID ? nte_reads::reject_cutoff(ctx) : 0;
	auto run_batch = [&](const char* text, uint64_t len, int where) {
		return pass == NTEDIT_READS_PASS_COUNT  ? ntedit_hip_sketch_count(ctx, text, len, where)
		       : pass == NTEDIT_READS_PASS_HIST ? ntedit_hip_sketch_histogram(ctx, text, len, where)
		       : rmin                           ? ntedit_hip_filter_insert_solid2(ctx, text, len, where, cmin, rmin)
		                                        : ntedit_hip_filter_insert_solid(ctx, NTEDIT_FILTER_PRIMARY, text, len, where, cmin);
	};
	// the host parser over some ranges (all of them, without --gpu_parse)
	auto host_pass = [&](const std::vector<Range>& rs, uint64_t* rs_starts, uint64_t* rs_nexts) {
		BatchFeeder feed(rs, keep, (size_t)batch_bytes, rs_starts, rs_nexts);
		for (;;) {
			Batch* b = feed.take();
			if (!b) {
				return pfail(ctx, NTEDIT_E_IO, feed.error());
			}
			const auto g0 = std::chrono::steady_clock::now();
			const int rc = b->len ? run_batch(b->p, b->len, NTEDIT_HIP_BASES_HOST) : 0; // (an input without any read of k bases ends in an empty batch)
			if (rc) {
				return pfail(ctx, rc, ntedit_hip_reads_last_error(ctx));
			}
			gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
			bases += b->bases;
			const bool last = b->last;
			feed.give_back(b);
			if (last) {
				return 0;
			}
		}
	};
	if (!nte_reads::parse_is_on(ctx)) {
		for (const Range& r : ranges) { // (the host parser would read whatever '@' and '>' bytes the binary stream holds)
			if (ntedit_hip_reads_is_bam(r.path)) {
				return pfail(ctx, NTEDIT_E_ARG, std::string("--reads ") + r.path + ": BAM needs --gpu_parse");
			}
		}
		const int rc = host_pass(ranges, starts, nexts);
		if (rc) {
			return rc;
		}
	} else {
		ntedit_hip_reads_parse_stats& info = *nte_reads::parse_info(ctx);
		info = ntedit_hip_reads_parse_stats();
		ntedit_hip_reads_inflate_stats& zinfo = *nte_reads::inflate_info(ctx);
		zinfo = ntedit_hip_reads_inflate_stats();
		ntedit_hip_reads_bam_stats& binfo = *nte_reads::bam_info(ctx);
		binfo = ntedit_hip_reads_bam_stats();
		for (uint32_t i = 0; i < n; i++) {
			const Range& r = ranges[i];
			struct stat sb;
			const bool regular = stat(r.path, &sb) == 0 && S_ISREG(sb.st_mode);
			if (regular && r.begin == 0 && r.end == WHOLE && is_bgzf(r.path)) {
				// a BGZF file, whole: shipped compressed, inflated and cut on the device.  `base` is the inflated
				// offset of the raw buffer's first byte, always a record start; `tail` the bytes carried behind a cut.
				zinfo.files++;
				// a BAM takes the same loop: its walk in place of the last record start, its decode in place of the
				// text parser.  There is no host parser to hand it back to: what the BGZF path hands back fails the pass.
				const bool bam = ntedit_hip_reads_is_bam(r.path) != 0;
				bool bam_header_done = false;
				auto bam_fail = [&](const std::string& what, uint64_t at) {
					return pfail(ctx, NTEDIT_E_IO, std::string(r.path) + ": BAM: " + what + " at inflated offset " + std::to_string(at));
				};
				if (bam) {
					binfo.files++;
				}
				uint64_t base = 0, tail = 0;
				bool handed_back = false;
				{
					BgzfFeeder feed(r.path, (size_t)batch_bytes);
					BgzfChunk* cur = feed.take();
					int which = 0;
					if (!cur) {
						return pfail(ctx, NTEDIT_E_IO, feed.error());
					}
					if (nte_reads::inflate_copy_begin(ctx, which, cur->p, cur->len, cur->m, cur->n_members) != 0) {
						return NTEDIT_E_DEVICE;
					}
					while (cur) {
						// the copy of chunk i + 1 runs while chunk i is inflated, parsed and counted
						BgzfChunk* next = nullptr;
						if (!cur->last) {
							if (!(next = feed.take())) {
								(void)nte_reads::inflate_copy_wait(ctx, which);
								return pfail(ctx, NTEDIT_E_IO, feed.error());
							}
							if (nte_reads::inflate_copy_begin(ctx, which ^ 1, next->p, next->len, next->m, next->n_members) != 0) {
								(void)nte_reads::inflate_copy_wait(ctx, which);
								return NTEDIT_E_DEVICE;
							}
						}
						const auto g0 = std::chrono::steady_clock::now();
						const char* raw = nullptr;
						uint64_t bad = 0, cut = 0;
						uint32_t reason = 0, broken = 0;
						int rc = nte_reads::inflate_copied(ctx, which, cur->len, cur->m, cur->n_members, tail, cur->n_out, &raw, &bad, &reason);
						const uint64_t total = tail + cur->n_out, first_member = cur->first_member;
						const bool last = cur->last, whole = cur->whole;
						feed.give_back(cur); // (its copy is done: the reader may fill it again)
						if (rc == 0 && reason) {
							zinfo.bad_member = first_member + bad;
							zinfo.bad_reason = reason;
							(void)nte_reads::inflate_copy_wait(ctx, which ^ 1);
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
							(void)nte_reads::inflate_copy_wait(ctx, which ^ 1);
							return pfail(ctx, rc, ntedit_hip_reads_last_error(ctx));
						}
						gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
						if (bam && !res.clean) {
							(void)nte_reads::inflate_copy_wait(ctx, which ^ 1);
							return bam_fail(bres.broken & NTEDIT_BAM_BAD_MAGIC    ? "the header does not start with the BAM magic"
							                : bres.broken & NTEDIT_BAM_BAD_HEADER ? "a header with a negative length or an empty reference name"
							                : bres.broken & NTEDIT_BAM_BAD_SIZE   ? "a record with a block_size outside [0, 2^30), or a chunk of 2 GiB"
							                                                      : "a record whose parts do not fit its block_size",
							                base + bres.cut);
						}
						if (!res.clean) {
							info.fallback_chunks++;
							info.broken |= res.broken;
							handed_back = true;
							(void)nte_reads::inflate_copy_wait(ctx, which ^ 1); // (before the feeder frees the buffer it reads)
							break;
						}
						if (cut && !bam) { // (a BAM's chunks are the BAM counters': the text parser saw none of them)
							info.device_chunks++;
							info.raw_bytes += cut;
							info.text_bytes += res.text_len;
						}
						if (cut) {
							bases += res.bases;
						}
						// a chunk without a record start past its first byte grows by the next one (cut = 0: all is tail)
						if (cut && cut < total && nte_reads::inflate_carry(ctx, cut, total) != 0) {
							(void)nte_reads::inflate_copy_wait(ctx, which ^ 1);
							return NTEDIT_E_DEVICE;
						}
						base += cut;
						tail = total - cut;
						bam_header_done = bam_header_done || cut > 0; // (a header that does not fit gives cut 0)
						if (bam && last && !whole) {
							return bam_fail("what follows the last whole BGZF member is not one (a damaged or truncated file); the records end",
							                base);
						}
						if (bam && last && tail) {
							return bam_fail(std::to_string(tail) + " bytes are left over behind the last whole record (a truncated file)", base);
						}
						if (last && !whole) {
							handed_back = true; // what follows the members is not BGZF: the host parser's, from `base`
						}
						cur = next;
						which ^= 1;
					}
				}
				if (starts) {
					starts[i] = 0;
				}
				if (handed_back) {
					zinfo.handed_back++;
					zinfo.handed_back_at = base;
					Range rest = r;
					rest.skip = base;
					const int rc = host_pass({ rest }, nullptr, nexts ? nexts + i : nullptr);
					if (rc) {
						return rc;
					}
				} else if (nexts) {
					nexts[i] = base;
				}
				continue;
			}
			if (regular && ntedit_hip_reads_is_bam(r.path)) {
				return pfail(ctx, NTEDIT_E_ARG, std::string(r.path) + ": a BAM file is read whole, not in ranges");
			}
			if (!regular || is_gzip(r.path)) { // a gzip file (or what the host parser will refuse in its own words)
				info.host_files++;
				const int rc = host_pass({ r }, starts ? starts + i : nullptr, nexts ? nexts + i : nullptr);
				if (rc) {
					return rc;
				}
				continue;
			}
			// the range's first record start as the host parser finds it, and where its last chunk ends: the first
			// record start at or past `end` by the same rule
			const uint64_t size = (uint64_t)sb.st_size;
			uint64_t start = 0, stop = size;
			std::string why;
			if ((r.begin > 0 && !find_record_start(r.path, r.begin, &start, &why)) ||
			    (r.end < size && r.end > 0 && !find_record_start(r.path, r.end, &stop, &why))) {
				return pfail(ctx, NTEDIT_E_IO, why);
			}
			if (starts) {
				starts[i] = start;
			}
			if (start >= r.end || start >= size) {
				if (nexts) {
					nexts[i] = start; // no record starts in the range
				}
				continue;
			}
			uint64_t handed_back = WHOLE; // where an unclean chunk started
			{
				RawFeeder feed(r.path, start, stop, (size_t)batch_bytes);
				RawChunk* cur = feed.take();
				int which = 0;
				if (!cur) {
					return pfail(ctx, NTEDIT_E_IO, feed.error());
				}
				if (nte_reads::parse_copy_begin(ctx, which, cur->p, cur->len) != 0) {
					return NTEDIT_E_DEVICE;
				}
				while (cur) {
					// the copy of chunk i + 1 runs while chunk i is parsed and counted
					RawChunk* next = nullptr;
					if (!cur->last) {
						if (!(next = feed.take())) {
							(void)nte_reads::parse_copy_wait(ctx, which);
							return pfail(ctx, NTEDIT_E_IO, feed.error());
						}
						if (nte_reads::parse_copy_begin(ctx, which ^ 1, next->p, next->len) != 0) {
							(void)nte_reads::parse_copy_wait(ctx, which);
							return NTEDIT_E_DEVICE;
						}
					}
					const auto g0 = std::chrono::steady_clock::now();
					const char* text = nullptr;
					ntedit_hip_reads_parse_result res;
					int rc = nte_reads::parse_copied(ctx, which, cur->len, keep, &text, &res);
					const uint64_t off = cur->off, len = cur->len;
					feed.give_back(cur); // (its copy is done: the reader may fill it again)
					if (rc == 0 && res.clean && res.text_len) {
						rc = run_batch(text, res.text_len, NTEDIT_HIP_BASES_DEVICE);
					}
					if (rc) {
						(void)nte_reads::parse_copy_wait(ctx, which ^ 1);
						return pfail(ctx, rc, ntedit_hip_reads_last_error(ctx));
					}
					gpu_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
					if (!res.clean) {
						info.fallback_chunks++;
						info.broken |= res.broken;
						handed_back = off;
						(void)nte_reads::parse_copy_wait(ctx, which ^ 1); // (before the feeder frees the buffer it reads)
						break;
					}
					info.device_chunks++;
					info.raw_bytes += len;
					info.text_bytes += res.text_len;
					bases += res.bases;
					cur = next;
					which ^= 1;
				}
			}
			if (handed_back != WHOLE) {
				// the rest of the range, from that chunk's first byte, with kseq's rules
				Range rest = r;
				rest.begin = handed_back;
				rest.exact = true;
				const int rc = host_pass({ rest }, nullptr, nexts ? nexts + i : nullptr);
				if (rc) {
					return rc;
				}
			} else if (nexts) {
				nexts[i] = stop;
			}
		}
	}
	if (stats) {
		stats->bases = bases;
		stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		stats->ms_gpu = gpu_ms;
	}
	return 0;
}

int
ntedit_hip_reads_range_text(const char* path, uint64_t begin, uint64_t end, char* out, uint64_t cap, uint64_t* len,
                            uint64_t* reads, uint64_t* start, uint64_t* next)
{
	if (!path || !len || !reads || !start || !next || begin > end || (cap && !out)) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_range_text: bad argument");
	}
	uint64_t used = 0, count = 0;
	std::string why;
	const bool ok = read_range(path, begin, end, [&](const std::string& seq) {
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

namespace {

// the build's console lines; a rank's share of a sharded build (ranges) names the rank on its pass and store lines, and
// only rank 0 (the one process of an unsharded build is rank 0) says what every rank decides alike
struct BuildLog
{
	const ntedit_hip_reads_build_args* a;
	bool first_only = false;
	bool ranged() const { return a->begins != nullptr; }
	void rank_info(const std::string& s) const
	{
		info(ranged() ? "rank " + std::to_string(a->rank) + "/" + std::to_string(a->world) + ": " + s : s);
	}
	void info(const std::string& s) const { line(0, s); }
	void out(const std::string& s) const { line(1, s); }
	void line(int to_stdout, const std::string& s) const
	{
		if (a->log && !(first_only && a->rank != 0)) {
			a->log(a->user, to_stdout, s.c_str());
		}
	}
};

// one pass, over the ranges (the files whole) or over the resident store (the store's bases: pass 1's), and its line
// (the large-run tests read it).  Pass 1 reads the store only when the build began with one (r->from_store, set by
// stage_count from the store's state at entry); the later passes whenever the store is ON.
int
build_pass(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, int pass, ntedit_hip_reads_build_result* r, uint64_t* starts,
           uint64_t* nexts)
{
	static const char* const names[] = { "1 (count)", "H (histogram)", "2 (solid k-mers)" };
	const BuildLog lg{ a };
	ntedit_hip_reads_pass_stats& st = r->pass[pass];
	std::string what;
	int rc;
	const bool from_store = r->from_store != 0;
	uint64_t store_bases = 0; // of a store the build began with: its bytes, reads and separators (nobody kept its reads' bases)
	if (from_store) {
		ntedit_hip_resident_stats ss;
		if (ntedit_hip_resident_info(ctx, &ss) != 0) {
			return NTEDIT_E_DEVICE;
		}
		store_bases = ss.bases;
	}
	const bool read_files = r->store_state != NTEDIT_RESIDENT_ON || (pass == NTEDIT_READS_PASS_COUNT && !from_store);
	if (!read_files) {
		const auto t0 = std::chrono::steady_clock::now();
		rc = pass == NTEDIT_READS_PASS_COUNT  ? ntedit_hip_resident_count(ctx)
		     : pass == NTEDIT_READS_PASS_HIST ? ntedit_hip_resident_histogram(ctx)
		     : a->reject_cmin               ? ntedit_hip_resident_insert_solid2(ctx, r->cmin, a->reject_cmin)
		                                    : ntedit_hip_resident_insert_solid(ctx, NTEDIT_FILTER_PRIMARY, r->cmin);
		st.bases = from_store ? store_bases : r->pass[NTEDIT_READS_PASS_COUNT].bases;
		st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		st.ms_gpu = st.ms_wall;
		what = std::to_string(r->store_batches) + " batches of the resident store";
	} else {
		const std::vector<uint64_t> begins(a->n_files, 0), ends(a->n_files, WHOLE);
		rc = ntedit_hip_reads_pass(ctx, pass, a->files, lg.ranged() ? a->begins : begins.data(), lg.ranged() ? a->ends : ends.data(),
		                           a->n_files, a->batch_bytes, r->cmin, &st, starts, nexts);
		what = std::to_string(a->n_files) + " ranges";
	}
	if (rc != 0) {
		return NTEDIT_E_IO; // (the message is the pass's)
	}
	char line[256];
	snprintf(line, sizeof line, "Pass %s: %llu bases, %.1f ms, %.3f Gbases/s (GPU calls %.1f ms, %.3f Gbases/s)", names[pass],
	         (unsigned long long)st.bases, st.ms_wall, st.ms_wall > 0 ? st.bases / st.ms_wall / 1e6 : 0.0, st.ms_gpu,
	         st.ms_gpu > 0 ? st.bases / st.ms_gpu / 1e6 : 0.0);
	lg.rank_info(lg.ranged() || from_store ? line + (", " + what) : line);
	ntedit_hip_reads_parse_stats ps;
	if (a->device_parse && read_files && ntedit_hip_reads_parse_info(ctx, &ps) == 0) {
		// the pass's one line about --gpu_parse (the tests read it)
		std::string l = "--gpu_parse: " + std::to_string(ps.device_chunks) + " chunks parsed on the device (" + std::to_string(ps.raw_bytes) +
		                " raw bytes, " + std::to_string(ps.text_bytes) + " text bytes, ";
		snprintf(line, sizeof line, "%.1f ms in the parse kernels)", ps.ms_kernels);
		l += line;
		if (ps.fallback_chunks) {
			static const char* const rules[] = { "the first byte is neither '>' nor '@'", "a carriage return", "an empty line",
				                                 "a sequence line that starts with '>', '+' or '@'", "FASTQ lines not a multiple of 4",
				                                 "a FASTQ header without '@'", "a FASTQ line 3 without '+'",
				                                 "a quality line not as long as its sequence", "more than one line per 8 bytes",
				                                 "a chunk of 2 GiB or more" };
			std::string whys;
			for (int b = 0; b < 10; b++) {
				if (ps.broken & (1u << b)) {
					whys += (whys.empty() ? "" : "; ") + std::string(rules[b]);
				}
			}
			l += ", " + std::to_string(ps.fallback_chunks) + " unclean chunks sent the rest of their ranges to the host parser (" + whys + ")";
		}
		if (ps.host_files) {
			l += ", " + std::to_string(ps.host_files) + " gzip inputs stay with the host parser";
		}
		lg.rank_info(l);
		ntedit_hip_reads_inflate_stats zs;
		if (ntedit_hip_reads_inflate_info(ctx, &zs) == 0 && zs.files) {
			// ... and one about its BGZF inputs (the tests read it)
			l = "--gpu_parse: BGZF: " + std::to_string(zs.members) + " members of " + std::to_string(zs.files) +
			    (zs.files == 1 ? " file" : " files") + " inflated on the device (" + std::to_string(zs.comp_bytes) +
			    " compressed bytes, " + std::to_string(zs.raw_bytes) + " inflated bytes, ";
			snprintf(line, sizeof line, "%.1f ms in the inflate kernels), ", zs.ms_kernels);
			l += line + std::to_string(zs.handed_back) + (zs.handed_back == 1 ? " file" : " files") + " handed back";
			if (zs.handed_back) {
				l += " to the host parser (the last at inflated offset " + std::to_string(zs.handed_back_at) + ")";
			}
			l += "; " + std::to_string(ps.host_files) + " gzip inputs stay with the host parser";
			lg.rank_info(l);
		}
		ntedit_hip_reads_bam_stats bs;
		if (ntedit_hip_reads_bam_info(ctx, &bs) == 0 && bs.files) {
			// ... and one about its BAM inputs (the tests read it)
			l = "--gpu_parse: BAM: " + std::to_string(bs.records) + " records of " + std::to_string(bs.files) +
			    (bs.files == 1 ? " file" : " files") + " walked on the device (" + std::to_string(bs.kept) + " kept, " +
			    std::to_string(bs.skipped_flag) + " secondary or supplementary, " + std::to_string(bs.skipped_short) + " too short; " +
			    std::to_string(bs.chunks) + " chunks, " + std::to_string(bs.segments) + " segments, " + std::to_string(bs.rewalked) +
			    " walked again by the stitch, ";
			snprintf(line, sizeof line, "%.1f ms in the walk kernels, %.1f ms in the decode kernels)", bs.ms_walk, bs.ms_decode);
			lg.rank_info(l + line);
		}
	}
	return 0;
}

// the end of a build: the sketch freed and the store with it, or (keep_store, the build succeeded and its store is ON)
// the counters alone released and the store kept for the next build
void
end_build(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, const ntedit_hip_reads_build_result* r, int rc)
{
	if (rc == 0 && a && r && a->keep_store && r->store_state == NTEDIT_RESIDENT_ON && ntedit_hip_sketch_reset(ctx, 0, 0, 0) == 0) {
		return;
	}
	ntedit_hip_sketch_free(ctx);
}

bool
bad_build_args(const ntedit_hip_reads_build_args* a, const ntedit_hip_reads_build_result* r)
{
	return !a || !r || (a->n_files && !a->files) || (a->begins && !a->ends) || a->batch_bytes < 4096 ||
	       (!a->solid && (a->cmin < 1 || a->cmin > 255)) || (a->bf_bytes == 0 && !a->solid && !a->hist_path) ||
	       (a->reject_cmin && (a->reject_cmin > 255 || a->counts || (a->reject_bf_bytes == 0 && !a->solid && !a->hist_path)));
}

} // namespace

extern "C" {

int
ntedit_hip_reads_stage_count(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r,
                             uint64_t* starts, uint64_t* nexts)
{
	if (!ctx || bad_build_args(a, r)) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_stage_count: bad argument");
	}
	const BuildLog lg{ a };
	*r = ntedit_hip_reads_build_result();
	ntedit_hip_reads_set_device_parse(ctx, a->device_parse);
	// a store an earlier build left ON (keep_store): this build's three passes read it, and no file is opened
	ntedit_hip_resident_stats at_entry;
	const bool from_store = !lg.ranged() && a->use_store && ntedit_hip_resident_info(ctx, &at_entry) == 0 &&
	                        at_entry.state == NTEDIT_RESIDENT_ON;
	if (from_store) {
		if (ntedit_hip_sketch_reset(ctx, a->sketch_counters, a->hash_num, a->k) != 0) {
			return NTEDIT_E_DEVICE; // (the message is sketch_reset's)
		}
		r->from_store = 1;
		r->store_state = at_entry.state; // (build_pass routes by both)
		r->store_batches = at_entry.batches;
	} else {
		if (!lg.ranged() && ntedit_hip_sketch_alloc(ctx, a->sketch_counters, a->hash_num, a->k) != 0) {
			return NTEDIT_E_DEVICE; // (the message is sketch_alloc's)
		}
		if (ntedit_hip_reads_set_min_read(ctx, a->min_read) != 0) {
			return NTEDIT_E_DEVICE;
		}
		if (a->use_store && ntedit_hip_resident_begin(ctx, a->store_cap) != 0) {
			return NTEDIT_E_DEVICE;
		}
	}
	lg.rank_info("Pass 1: counting k-mers");
	if (build_pass(ctx, a, NTEDIT_READS_PASS_COUNT, r, starts, nexts) != 0) {
		return NTEDIT_E_IO;
	}
	if (a->use_store) {
		ntedit_hip_resident_stats ss;
		if (ntedit_hip_resident_info(ctx, &ss) != 0) {
			return NTEDIT_E_DEVICE;
		}
		r->store_state = ss.state;
		r->store_bytes = ss.bytes;
		r->store_batches = ss.batches;
		const std::string later = a->solid || a->hist_path ? "the histogram pass and pass 2" : "pass 2";
		if (from_store) {
			lg.rank_info("Resident store: kept from the build before, " + std::to_string(ss.batches) + " batches, " + std::to_string(ss.bytes) +
			             " bytes of HBM (3 bits per base); every pass of this build reads it, no file is opened");
		} else if (ss.state == NTEDIT_RESIDENT_ON) {
			lg.rank_info("Resident store: " + std::to_string(ss.batches) + " batches, " + std::to_string(ss.bytes) +
			             " bytes of HBM (3 bits per base); " + later + " read it");
		} else {
			lg.rank_info(std::string("Resident store: released (") +
			             (ss.state == NTEDIT_RESIDENT_OVER_CAP ? "the reads would pass its cap of " + std::to_string(ss.cap) + " bytes"
			                                                      : std::string("a device allocation failed")) +
			             "); " + later + " read the files");
		}
	}
	return 0;
}

int
ntedit_hip_reads_stage_histogram(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r,
                                 uint64_t occ[256])
{
	if (!ctx || bad_build_args(a, r) || !occ) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_stage_histogram: bad argument");
	}
	const BuildLog lg{ a };
	ntedit_hip_reads_set_device_parse(ctx, a->device_parse);
	lg.rank_info("Histogram pass: the k-mer histogram of the sketch's estimates");
	if (build_pass(ctx, a, NTEDIT_READS_PASS_HIST, r, nullptr, nullptr) != 0) {
		return NTEDIT_E_IO;
	}
	return ntedit_hip_sketch_histogram_download(ctx, occ) != 0 ? NTEDIT_E_DEVICE : 0;
}

int
ntedit_hip_reads_stage_decide(const ntedit_hip_reads_build_args* a, const uint64_t occ[256], ntedit_hip_reads_build_result* r)
{
	if (bad_build_args(a, r) || (!occ && (a->solid || a->bf_bytes == 0 || (a->reject_cmin && a->reject_bf_bytes == 0)))) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_stage_decide: bad argument");
	}
	const BuildLog lg{ a, true };
	r->cmin = a->cmin;
	r->bf_bytes = a->bf_bytes;
	r->reject_bf_bytes = a->reject_cmin ? a->reject_bf_bytes : 0;
	const std::string reject = "--reject_cutoff " + std::to_string(a->reject_cmin);
	if (occ) {
		uint64_t f[256], F0 = 0, F1 = 0;
		ntedit_hip_reads_hist_summary(occ, f, &F0, &F1);
		lg.info("k-mer histogram: F1 = " + std::to_string(F1) + " (k-mers), F0 = " + std::to_string(F0) + " (distinct k-mers)");
		// written first: a refused --solid still leaves the histogram to look at
		if (a->hist_path && a->rank == 0) {
			if (ntedit_hip_reads_write_hist(a->hist_path, f, F0, F1) != 0) {
				return pfail(nullptr, NTEDIT_E_IO, std::string("cannot write ") + a->hist_path);
			}
			lg.info(std::string("Histogram written to ") + a->hist_path);
		}
		if (a->solid) {
			if (ntedit_hip_reads_solid_cutoff(f, &r->cmin) != 0) {
				return pfail(nullptr, NTEDIT_E_ARG, "--solid: the k-mer histogram has no valley after the error peak (no c with "
				                                    "f[c+1] > f[c]); pass -c");
			}
			lg.info("--solid: minimum k-mer count " + std::to_string(r->cmin));
			if (a->reject_cmin && a->reject_cmin <= r->cmin) {
				return pfail(nullptr, NTEDIT_E_ARG, reject + ": the reject count must be above the minimum count, and --solid found " +
				                                        std::to_string(r->cmin));
			}
		}
		if (a->reject_cmin && a->reject_bf_bytes == 0) {
			uint64_t num_elements = 0;
			for (uint64_t c = a->reject_cmin; c < 256; c++) {
				num_elements += f[c];
			}
			r->reject_bf_bytes = ntedit_hip_reads_bf_size(num_elements, a->hash_num, a->fpr);
			lg.info("Reject filter sized from the k-mer histogram: --reject_num_elements " + std::to_string(num_elements) + " (k-mers at " +
			        std::to_string(a->reject_cmin) + " or above), " + std::to_string(r->reject_bf_bytes) + " bytes");
			if (r->reject_bf_bytes == 0) {
				return pfail(nullptr, NTEDIT_E_ARG, "The reject filter would be empty (no k-mer at " + reject + " or above).");
			}
			lg.out("Reject BF size (bytes): " + std::to_string(r->reject_bf_bytes));
		}
		if (a->bf_bytes == 0) {
			uint64_t num_elements = 0;
			for (uint64_t c = r->cmin; c < 256; c++) {
				num_elements += f[c];
			}
			r->bf_bytes = ntedit_hip_reads_bf_size(num_elements, a->hash_num, a->fpr);
			lg.info("Sized from the k-mer histogram: --num_elements " + std::to_string(num_elements) + " (k-mers at " +
			        std::to_string(r->cmin) + " or above), " + std::to_string(r->bf_bytes) + " bytes");
			if (r->bf_bytes == 0) {
				return pfail(nullptr, NTEDIT_E_ARG, "The output filter would be empty (no k-mer at the minimum count or above).");
			}
			lg.out("BF size (bytes): " + std::to_string(r->bf_bytes));
		}
	}
	if (r->bf_bytes == 0) {
		return pfail(nullptr, NTEDIT_E_ARG, "The output filter would be empty (--bf 0 or --num_elements too small).");
	}
	if (a->reject_cmin && a->reject_cmin <= r->cmin) {
		return pfail(nullptr, NTEDIT_E_ARG, reject + ": the reject count must be above the minimum count " + std::to_string(r->cmin));
	}
	if (a->reject_cmin && r->reject_bf_bytes == 0) {
		return pfail(nullptr, NTEDIT_E_ARG, "The reject filter would be empty (--reject_bf 0 or --reject_num_elements too small).");
	}
	return 0;
}

int
ntedit_hip_reads_stage_insert(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r)
{
	if (!ctx || bad_build_args(a, r) || r->bf_bytes == 0 || r->cmin < 1 || r->cmin > 255 ||
	    (a->reject_cmin && (r->reject_bf_bytes == 0 || a->reject_cmin <= r->cmin))) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_stage_insert: bad argument");
	}
	const BuildLog lg{ a };
	if (lg.ranged()) { // (the filter is the one the caller adopted in the PRIMARY slot)
	} else if (a->counts) {
		if (ntedit_hip_filter_alloc_counting(ctx, NTEDIT_FILTER_PRIMARY, r->bf_bytes, a->hash_num, a->k) != 0) {
			return NTEDIT_E_DEVICE;
		}
	} else if (ntedit_hip_filter_alloc(ctx, NTEDIT_FILTER_PRIMARY, r->bf_bytes, a->hash_num, a->k) != 0) {
		return pfail(ctx, NTEDIT_E_DEVICE, ntedit_hip_last_error(ctx));
	}
	// the reject filter: plain, same k and hash count, in the SECONDARY slot (a sharded build: the adopted one)
	if (a->reject_cmin && !lg.ranged() &&
	    ntedit_hip_filter_alloc(ctx, NTEDIT_FILTER_SECONDARY, r->reject_bf_bytes, a->hash_num, a->k) != 0) {
		return pfail(ctx, NTEDIT_E_DEVICE, ntedit_hip_last_error(ctx));
	}
	if (a->reject_cmin && ntedit_hip_reads_set_reject_cutoff(ctx, a->reject_cmin) != 0) { // (for a pass 2 over the files)
		return NTEDIT_E_ARG;
	}
	ntedit_hip_reads_set_device_parse(ctx, a->device_parse);
	lg.rank_info("Pass 2: inserting k-mers seen at least " + std::to_string(r->cmin) + " times" +
	             (a->reject_cmin ? ", and into the reject filter those seen at least " + std::to_string(a->reject_cmin) + " times" : ""));
	const int rc = build_pass(ctx, a, NTEDIT_READS_PASS_SOLID, r, nullptr, nullptr);
	end_build(ctx, a, r, rc);
	return rc;
}

int
ntedit_hip_reads_build(ntedit_hip_ctx* ctx, const ntedit_hip_reads_build_args* a, ntedit_hip_reads_build_result* r)
{
	const auto t0 = std::chrono::steady_clock::now();
	uint64_t occ[256], nonzero = 0, counters = 0;
	const bool hist = a && (a->solid || a->hist_path);
	int rc = ntedit_hip_reads_stage_count(ctx, a, r, nullptr, nullptr);
	if (rc == 0 && ntedit_hip_sketch_occupancy(ctx, &nonzero, &counters) != 0) {
		rc = NTEDIT_E_DEVICE;
	}
	if (rc == 0) {
		std::ostringstream o;
		o << "Sketch occupancy: " << nonzero << " / " << counters << " counters (" << (double)nonzero / (double)counters << ")";
		BuildLog{ a }.out(o.str());
		if (a->sketch_path && ntedit_hip_sketch_save_file(ctx, a->sketch_path) != 0) {
			rc = NTEDIT_E_IO;
		}
	}
	if (rc == 0 && hist) {
		rc = ntedit_hip_reads_stage_histogram(ctx, a, r, occ);
	}
	if (rc == 0 && (rc = ntedit_hip_reads_stage_decide(a, hist ? occ : nullptr, r)) != 0) {
		pfail(ctx, rc, ntedit_hip_reads_last_error(nullptr)); // (the message of a call without a context, to the context's)
	}
	if (rc == 0) {
		rc = ntedit_hip_reads_stage_insert(ctx, a, r);
	}
	if (ctx) {
		end_build(ctx, a, r, rc);
	}
	if (r) {
		r->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	return rc;
}

} // extern "C"

extern "C" {

// ntCard's histogram file: "F1\t<n>", "F0\t<n>", then "c\tf[c]" for c = 1..255 (zeros included)
int
ntedit_hip_reads_write_hist(const char* path, const uint64_t f[256], uint64_t F0, uint64_t F1)
{
	if (!path || !f) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_write_hist: bad argument");
	}
	FILE* fp = fopen(path, "w");
	if (!fp) {
		return pfail(nullptr, NTEDIT_E_IO, std::string("cannot write ") + path);
	}
	fprintf(fp, "F1\t%llu\nF0\t%llu\n", (unsigned long long)F1, (unsigned long long)F0);
	for (int c = 1; c < 256; c++) {
		fprintf(fp, "%d\t%llu\n", c, (unsigned long long)f[c]);
	}
	const bool ok = !ferror(fp);
	if (fclose(fp) != 0 || !ok) {
		return pfail(nullptr, NTEDIT_E_IO, std::string("cannot write ") + path);
	}
	return 0;
}

} // extern "C"
