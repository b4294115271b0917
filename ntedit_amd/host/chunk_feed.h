// chunk_feed.h -- how the filter builds' passes get their input: a file becomes chunks in page-locked memory, made by one
// producer thread while the GPU works on the chunks before, and the pass overlaps the copy of chunk i + 1 with its work
// on chunk i.  Written once for ntedit_hip_reads_pass (reads_pass.cpp) and ntedit_hip_genome_pass (genome_pass.cpp):
//
//   Pinned       a page-locked buffer that grows; the caller says by how much
//   Feed<Chunk>  the queue: two chunks, one producer thread, take / give_back
//   producers    parsed batches (batch_add; the parser that calls it is reads_pass.cpp's), raw chunks of a plain file cut
//                at record starts or anywhere (RawProducer), whole BGZF members still compressed (BgzfGather, BgzfProducer)
//   overlap      the pass's loop over a feed, and the one place that waits for a copy in flight before its buffer can go
//
// Plain C++17 and nothing of HIP: tests/feed/feed_host.cpp builds this header alone, under the address, undefined-behaviour
// and thread sanitizers, with malloc behind ntedit_hip_host_alloc.
#pragma once

#include "../../include/ntedit_hip.h"
#include "bgzf_walk.h"

#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace nte_host {

const size_t NO_CUT = ~(size_t)0;
const size_t CHUNK_MAX = 1u << 30;   // (the device parsers take chunks below 2^31 bytes)
const unsigned RAW_READERS = 4;      // threads that pread slices of one chunk
const size_t RAW_SLICE_MIN = 4u << 20;
const char* const NO_PINNED = "cannot allocate page-locked host memory";

struct Pinned
{
	char* p = nullptr;
	size_t cap = 0;
	Pinned() = default;
	Pinned(const Pinned&) = delete;
	Pinned& operator=(const Pinned&) = delete;
	~Pinned() { ntedit_hip_host_free(p); }
	// room for `need` bytes, the first `keep` kept; a buffer that has to grow asks the allocator for exactly `need`
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

// Two chunks between one producer thread and one consumer.  `produce(feed)` runs on the thread: it fills what get_free()
// gives it (nullptr: the feed is being torn down, stop), queues it with put_full(), and returns after its last chunk or
// after fail().  The consumer's take() hands out what is queued, in order, and only then says that nothing follows
// (nullptr; error() is why, empty when the producer simply ended); what it took it gives back once no copy reads it.
template <class Chunk> class Feed
{
  public:
	template <class Producer> explicit Feed(Producer produce)
	{
		for (Chunk& c : chunks_) {
			free_.push_back(&c);
		}
		th_ = std::thread([this, produce = std::move(produce)]() mutable {
			produce(*this);
			end_(nullptr);
		});
	}
	~Feed()
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			stop_ = true;
		}
		cv_.notify_all();
		th_.join(); // (then the chunks' buffers go)
	}
	Chunk* take()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [this] { return !full_.empty() || ended_; });
		if (full_.empty()) {
			return nullptr;
		}
		Chunk* c = full_.front();
		full_.pop_front();
		return c;
	}
	void give_back(Chunk* c)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			free_.push_back(c);
		}
		cv_.notify_all();
	}
	const std::string& error() const { return err_; } // (after take() returned nullptr)

	// the producer's side
	Chunk* get_free()
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [this] { return !free_.empty() || stop_; });
		if (stop_) {
			return nullptr;
		}
		Chunk* c = free_.front();
		free_.pop_front();
		return c;
	}
	void put_full(Chunk* c)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			full_.push_back(c);
		}
		cv_.notify_all();
	}
	void fail(const std::string& why) { end_(&why); }

  private:
	void end_(const std::string* why)
	{
		{
			std::lock_guard<std::mutex> lk(mu_);
			if (why && !ended_) {
				err_ = *why;
			}
			ended_ = true;
		}
		cv_.notify_all();
	}

	Chunk chunks_[2];
	std::deque<Chunk*> free_, full_;
	bool stop_ = false, ended_ = false;
	std::string err_;
	std::mutex mu_;
	std::condition_variable cv_;
	std::thread th_;
};

// ------------------------------------------------------------------ the pass's loop
// The copy of chunk i + 1 into side `which ^ 1` runs while chunk i, copied into side `which`, is worked on:
//   begin(chunk, which)            starts the chunk's copy; non-zero: the pass fails with it
//   work(chunk, which, release)    waits for that copy and does the chunk's work.  release() gives the chunk back to the
//                                  producer and may be called as soon as the copy is done (after it the chunk is not the
//                                  consumer's to read); a chunk not released by then is given back when work returns 0.
//                                  0: go on; OVERLAP_STOP: leave the rest of the feed alone (a hand-back); else: failed
//   wait(which)                    waits for the copy last begun into that side
// Returns 0 after the chunk marked `last` (or after a producer that ended without one), OVERLAP_STOP, OVERLAP_FEED when
// the producer failed (feed.error()), or what begin or work failed with.  However it returns, both sides' copies have
// been waited for first: no page-locked buffer is refilled by the producer or freed by ~Feed while a copy reads it.
enum { OVERLAP_STOP = 1, OVERLAP_FEED = 2 };

template <class Chunk, class Begin, class Work, class Wait>
int
overlap(Feed<Chunk>& feed, Begin begin, Work work, Wait wait)
{
	struct Guard
	{
		Wait& wait;
		~Guard() { (void)wait(0), (void)wait(1); }
	} guard{ wait };
	Chunk* cur = feed.take();
	if (!cur) {
		return feed.error().empty() ? 0 : OVERLAP_FEED;
	}
	int which = 0;
	int rc = begin(*cur, which);
	while (rc == 0 && cur) {
		Chunk* next = nullptr;
		if (!cur->last) {
			if (!(next = feed.take())) {
				return feed.error().empty() ? 0 : OVERLAP_FEED;
			}
			if ((rc = begin(*next, which ^ 1)) != 0) {
				break;
			}
		}
		rc = work(*cur, which, [&] { feed.give_back(cur), cur = nullptr; });
		if (cur && rc == 0) {
			feed.give_back(cur);
		}
		cur = next;
		which ^= 1;
	}
	return rc;
}

// ------------------------------------------------------------------ producer: parsed batches
// reads separated by '\n' (no k-mer spans a separator), about batch_bytes of them a batch
struct Batch
{
	Pinned buf;
	size_t len = 0;
	uint64_t bases = 0;
	bool last = false;
};

inline Batch*
batch_begin(Feed<Batch>& feed)
{
	Batch* b = feed.get_free();
	if (b) {
		b->len = 0;
		b->bases = 0;
		b->last = false;
	}
	return b;
}

// one read into the batch *b, which is queued and replaced when the read does not fit; false: stop (the feed is being
// torn down: *b is nullptr; or it failed)
inline bool
batch_add(Feed<Batch>& feed, Batch*& b, const std::string& seq, unsigned k, size_t batch_bytes)
{
	if (seq.size() < k) { // no k-mer in it
		return true;
	}
	if (b->len && b->len + seq.size() + 1 > batch_bytes) {
		feed.put_full(b);
		if (!(b = batch_begin(feed))) {
			return false;
		}
	}
	const size_t need = b->len + seq.size() + 1;
	if (!b->buf.reserve(need > batch_bytes ? need : batch_bytes, b->len)) {
		feed.fail(NO_PINNED);
		return false;
	}
	memcpy(b->buf.p + b->len, seq.data(), seq.size());
	b->buf.p[b->len + seq.size()] = '\n';
	b->len += seq.size() + 1;
	b->bases += seq.size();
	return true;
}

// ------------------------------------------------------------------ producer: raw chunks of a plain file
// the last record start in buf(0, n) by find_record_start's rule (reads_pass.cpp) for a chunk of this kind: '>' at a line
// start, or an '@' line whose line + 2 (inside the buffer) starts with '+'; NO_CUT when there is none
inline size_t
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
		return NO_CUT;
	}
	size_t l1 = NO_CUT, l2 = NO_CUT; // the starts of the two lines behind the current one
	for (size_t end = n; end >= 2;) {
		const char* q = (const char*)memrchr(buf, '\n', end - 1);
		if (!q) {
			break;
		}
		const size_t cur = (size_t)(q - buf) + 1;
		if (l2 != NO_CUT && buf[cur] == '@' && buf[l2] == '+') {
			return cur;
		}
		l2 = l1;
		l1 = cur;
		end = cur;
	}
	return NO_CUT;
}

// file bytes [off, off + n) into p, by a few threads: raw reading has no order
inline bool
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

struct RawChunk
{
	Pinned buf;
	size_t len = 0;
	uint64_t off = 0; // of its first byte in the file
	bool last = false;
};

// The bytes [start, stop) of one plain file as chunks of about batch_bytes raw bytes.
//   CUT_RECORDS   (start a record start, stop a record start or the file's end) each chunk is cut at its last record
//                 start and the tail carried into the next; a chunk without a record start past its first byte grows by
//                 another batch_bytes (a record longer than a batch)
//   CUT_ANYWHERE  chunk i is the bytes [start + i * batch_bytes, ...): batch_bytes of them, or the rest
enum CutRule { CUT_RECORDS, CUT_ANYWHERE };

struct RawProducer
{
	const char* path;
	uint64_t start, stop;
	size_t batch_bytes;
	CutRule rule;

	void operator()(Feed<RawChunk>& feed) const
	{
		const size_t batch = batch_bytes < CHUNK_MAX ? batch_bytes : CHUNK_MAX;
		const int fd = open(path, O_RDONLY);
		if (fd < 0) {
			feed.fail(std::string("cannot open ") + path);
			return;
		}
		const std::string why = run(feed, fd, batch);
		close(fd);
		if (!why.empty()) {
			feed.fail(why);
		}
	}

	std::string run(Feed<RawChunk>& feed, int fd, size_t batch) const
	{
		std::vector<char> tail;
		for (uint64_t pos = start; pos < stop;) {
			RawChunk* b = feed.get_free();
			if (!b) {
				break;
			}
			size_t have = tail.size(), want = batch > have ? batch : have + batch;
			if (rule == CUT_ANYWHERE && (uint64_t)want > stop - pos) {
				want = (size_t)(stop - pos); // (a chunk's exact size; CUT_RECORDS asks for a batch even where the range ends before)
			}
			bool ok = b->buf.reserve(want, 0);
			if (ok && have) {
				memcpy(b->buf.p, tail.data(), have);
			}
			size_t cut = NO_CUT;
			while (ok) {
				if ((uint64_t)want > stop - pos) {
					want = (size_t)(stop - pos);
				}
				if (!pread_all(fd, b->buf.p + have, pos + have, want - have)) {
					return std::string(path) + ": read error";
				}
				have = want;
				if (pos + have == stop) {
					cut = have; // the range's last chunk ends where the range does
					break;
				}
				const int kind = (unsigned char)b->buf.p[0];
				cut = rule == CUT_RECORDS && (kind == '>' || kind == '@') ? last_record_start(b->buf.p, have, kind)
				                                                          : have; // (neither: unclean anyway)
				if (cut != NO_CUT) {
					break;
				}
				want = have + batch;
				ok = b->buf.reserve(want, have);
			}
			if (!ok) {
				return NO_PINNED;
			}
			tail.assign(b->buf.p + cut, b->buf.p + have);
			b->len = cut;
			b->off = pos;
			pos += cut;
			b->last = pos >= stop;
			feed.put_full(b);
		}
		return std::string();
	}
};

// ------------------------------------------------------------------ producer: BGZF files stay compressed
// A BGZF file as chunks of whole members whose ISIZE sum stays within batch_bytes (at least one member), compressed;
// nothing is inflated here.  The last chunk says how the members ended: with the file, or at something that is no
// (whole) BGZF member; it may hold no member at all.
struct BgzfChunk
{
	Pinned buf, table;
	size_t len = 0; // the compressed bytes of its members, buf.p[0 .. len)
	size_t n_members = 0;
	uint64_t n_out = 0;        // their ISIZE sum
	uint64_t first_member = 0; // the index of m()[0] in the file
	bool last = false;
	bool whole = true; // (last) the file ended behind a whole member
	ntedit_hip_bgzf_member* m() const { return (ntedit_hip_bgzf_member*)table.p; } // in_off / out_off from buf.p[0] / from m()[0]'s first byte
};

// the step of that: reads slabs, walks members, stops at the ISIZE budget and carries the compressed bytes it read
// behind the chunk's members into the next.  With a thread (BgzfProducer) or without one (the genome pass).
class BgzfGather
{
  public:
	BgzfGather(const char* path, size_t batch_bytes)
	    : path_(path), batch_(batch_bytes < CHUNK_MAX ? batch_bytes : CHUNK_MAX), slab_(batch_ / 4 + (128u << 10)), fd_(open(path, O_RDONLY))
	{
		struct stat sb;
		if (fd_ < 0 || fstat(fd_, &sb) != 0) {
			err_ = std::string("cannot open ") + path;
		} else {
			size_ = (uint64_t)sb.st_size;
		}
	}
	BgzfGather(const BgzfGather&) = delete;
	BgzfGather& operator=(const BgzfGather&) = delete;
	~BgzfGather()
	{
		if (fd_ >= 0) {
			close(fd_);
		}
	}
	const std::string& error() const { return err_; }

	// the file's next chunk into *b (a buffer grows to need + need / 2); false: the chunk before was the last, or error()
	bool next(BgzfChunk* b)
	{
		if (done_ || !err_.empty()) {
			return false;
		}
		size_t have = carry_.size(), walked = 0;
		bool ok = grow_(&b->buf, have > slab_ ? have : slab_, 0);
		if (ok && have) {
			memcpy(b->buf.p, carry_.data(), have);
		}
		b->n_members = 0;
		b->n_out = 0;
		b->first_member = member_;
		b->last = false;
		b->whole = true;
		while (ok) {
			ntedit_hip_bgzf_member one;
			uint64_t found = 0, used = 0;
			const int rc = bgzf_walk(b->buf.p + walked, have - walked, &one, 1, &found, &used);
			if (found) {
				if (b->n_members && b->n_out + one.n_out > batch_) {
					break; // the chunk is full
				}
				if (!(ok = grow_(&b->table, (b->n_members + 1) * sizeof one, b->n_members * sizeof one))) {
					break;
				}
				one.in_off += walked;
				one.out_off = b->n_out;
				b->m()[b->n_members++] = one;
				b->n_out += one.n_out;
				walked += (size_t)used;
				continue;
			}
			if (rc == NTEDIT_BGZF_NOT || pos_ + have >= size_) {
				// no member starts here, or the file ends inside one
				b->last = true;
				b->whole = rc != NTEDIT_BGZF_NOT && have == walked;
				break;
			}
			const size_t more = size_ - (pos_ + have) < slab_ ? (size_t)(size_ - (pos_ + have)) : slab_; // compressed bytes read at a time
			if (!(ok = grow_(&b->buf, have + more, have))) {
				break;
			}
			if (!pread_all(fd_, b->buf.p + have, pos_ + have, more)) {
				err_ = std::string(path_) + ": read error";
				return false;
			}
			have += more;
		}
		if (!ok) {
			err_ = NO_PINNED;
			return false;
		}
		carry_.assign(b->buf.p + walked, b->buf.p + have); // compressed bytes read behind the chunk's members
		b->len = walked;
		pos_ += walked;
		member_ += b->n_members;
		done_ = b->last;
		return true;
	}

  private:
	static bool grow_(Pinned* p, size_t need, size_t keep) { return need <= p->cap || p->reserve(need + need / 2, keep); }

	const char* path_;
	size_t batch_, slab_;
	int fd_;
	uint64_t size_ = 0, pos_ = 0, member_ = 0;
	std::vector<char> carry_;
	bool done_ = false;
	std::string err_;
};

struct BgzfProducer
{
	const char* path;
	size_t batch_bytes;

	void operator()(Feed<BgzfChunk>& feed) const
	{
		BgzfGather gather(path, batch_bytes);
		for (BgzfChunk* b; (b = feed.get_free()) && gather.next(b);) {
			const bool last = b->last;
			feed.put_full(b);
			if (last) {
				break;
			}
		}
		if (!gather.error().empty()) {
			feed.fail(gather.error());
		}
	}
};

// 0: plain, 1: a single-stream gzip file, 2: BGZF (bgzf_walk finds a member at byte 0, or finds its header and the end of
// what was read); *first: the file's first byte (-1: empty or unreadable)
inline int
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
	const int why = bgzf_walk(head, got, nullptr, 0, &found, &used);
	return got >= 28 && (why == NTEDIT_BGZF_FULL || (why == NTEDIT_BGZF_CUT && got == sizeof head)) ? 2 : 1;
}

} // namespace nte_host
