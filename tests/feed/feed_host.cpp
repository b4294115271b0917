// feed_host.cpp -- ntedit_amd/host/chunk_feed.h on the CPU, alone: the queue, the three producers and the overlap loop,
// with malloc behind the page-locked allocator.  tests/test_feed_cpu.py builds this program plain, with
// -fsanitize=address,undefined and with -fsanitize=thread, writes the input files, and compares what is printed here
// with its own restatement of the cut rules.  Nothing of the library is linked.
//
//   queue N [fail]                 a producer of N numbered chunks (then fail("boom")): what the consumer takes
//   abandon                        the consumer leaves after chunk 1 while the producer waits in get_free()
//   overlap N STOP_AT FAIL_AT BEGIN_FAIL_AT   the loop over N chunks with a pretended copy engine: a buffer that is
//                                  freed, or given back to the producer, while a copy reads it is a violation
//   batch FILE K BATCH             the lines of FILE through batch_add
//   raw FILE START STOP BATCH records|anywhere OUT     the raw chunks; their bytes, concatenated, to OUT
//   bgzf FILE BATCH thread|serial OUT                  the BGZF chunks and their members; their bytes to OUT
//   cut FILE KIND                  last_record_start of every prefix of FILE
#include "../../ntedit_amd/host/chunk_feed.h"

#include <atomic>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>

using namespace nte_host;

namespace {
std::mutex g_mu;
std::vector<size_t> g_allocs;     // the sizes asked of the allocator, in order
std::set<const void*> g_reading;  // buffers a pretended copy still reads
int g_violations = 0;
}

extern "C" void*
ntedit_hip_host_alloc(size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_allocs.push_back(bytes);
	return malloc(bytes); // (exactly: the sanitizer sees every byte past it)
}

extern "C" void
ntedit_hip_host_free(void* p)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_violations += p && g_reading.count(p);
	free(p);
}

namespace {

void
print_allocs()
{
	std::lock_guard<std::mutex> lk(g_mu);
	printf("allocs");
	for (size_t a : g_allocs) {
		printf(" %zu", a);
	}
	printf("\n");
}

struct Numbered
{
	Pinned buf;
	int id = -1;
	bool last = false;
};

// N numbered chunks, `last` on the last one; then, with `fail`, a failure
struct Counter
{
	int n;
	bool fail;
	std::atomic<int>* waiting_for = nullptr; // the chunk the producer is about to ask a free buffer for
	void operator()(Feed<Numbered>& feed) const
	{
		for (int i = 0; i < n; i++) {
			if (waiting_for) {
				waiting_for->store(i);
			}
			Numbered* c = feed.get_free();
			if (!c) {
				return;
			}
			{
				std::lock_guard<std::mutex> lk(g_mu);
				g_violations += c->buf.p && g_reading.count(c->buf.p); // (about to be filled again)
			}
			if (!c->buf.reserve(64, 0)) {
				feed.fail(NO_PINNED);
				return;
			}
			memset(c->buf.p, i & 255, 64);
			c->id = i;
			c->last = !fail && i == n - 1;
			feed.put_full(c);
		}
		if (fail) {
			feed.fail("boom");
		}
	}
};

int
run_queue(int n, bool fail)
{
	Feed<Numbered> feed(Counter{ n, fail });
	while (Numbered* c = feed.take()) {
		printf("chunk %d last %d byte %d\n", c->id, (int)c->last, (int)(unsigned char)c->buf.p[63]);
		const bool last = c->last;
		feed.give_back(c);
		if (last) {
			printf("end at last\n");
			return 0;
		}
	}
	printf("end error '%s'\n", feed.error().c_str());
	return 0;
}

int
run_abandon()
{
	std::atomic<int> waiting_for{ -1 };
	{
		Feed<Numbered> feed(Counter{ 1000, false, &waiting_for });
		Numbered* c = feed.take();
		printf("chunk %d\n", c->id);
		feed.give_back(c);
		c = feed.take();
		printf("chunk %d\n", c->id); // (kept: chunk 2 fills the other buffer, and no buffer is free for chunk 3)
		while (waiting_for.load() < 3) {
			std::this_thread::yield();
		}
	}
	printf("abandoned\n");
	return 0;
}

int
run_overlap(int n, int stop_at, int fail_at, int begin_fail_at)
{
	int rc, begun = 0, worked = 0, waits = 0;
	const void* side[2] = { nullptr, nullptr };
	{
		Feed<Numbered> feed(Counter{ n, false });
		auto begin = [&](const Numbered& c, int which) {
			if (c.id == begin_fail_at) {
				return -2;
			}
			std::lock_guard<std::mutex> lk(g_mu);
			g_reading.insert(side[which] = c.buf.p);
			begun++;
			return 0;
		};
		auto wait = [&](int which) {
			std::lock_guard<std::mutex> lk(g_mu);
			g_reading.erase(side[which]);
			side[which] = nullptr;
			waits++;
			return 0;
		};
		auto work = [&](const Numbered& c, int which, auto release) {
			const int id = c.id;
			if (id == fail_at) {
				return -5; // (before the copy was waited for: the chunk must not go back to the producer)
			}
			wait(which);
			release();
			{
				std::lock_guard<std::mutex> lk(g_mu);
				g_violations += g_reading.count(c.buf.p) != 0;
			}
			worked++;
			return id == stop_at ? (int)OVERLAP_STOP : 0;
		};
		rc = overlap(feed, begin, work, wait);
		std::lock_guard<std::mutex> lk(g_mu);
		g_violations += !g_reading.empty(); // (the feed goes next)
	}
	printf("overlap rc %d begun %d worked %d violations %d\n", rc, begun, worked, g_violations);
	return g_violations ? 1 : 0;
}

int
run_batch(const char* path, unsigned k, size_t batch_bytes)
{
	std::vector<std::string> lines;
	std::ifstream in(path);
	for (std::string l; std::getline(in, l);) {
		lines.push_back(l);
	}
	Feed<Batch> feed([&](Feed<Batch>& f) {
		Batch* b = batch_begin(f);
		for (const std::string& l : lines) {
			if (!b || !batch_add(f, b, l, k, batch_bytes)) {
				return;
			}
		}
		b->last = true;
		f.put_full(b);
	});
	while (Batch* b = feed.take()) {
		printf("batch len %zu bases %llu last %d\n", b->len, (unsigned long long)b->bases, (int)b->last);
		fwrite(b->buf.p, 1, b->len, stdout);
		const bool last = b->last;
		feed.give_back(b);
		if (last) {
			break;
		}
	}
	print_allocs();
	return 0;
}

int
run_raw(const char* path, uint64_t start, uint64_t stop, size_t batch_bytes, const std::string& rule, const char* out_path)
{
	FILE* out = fopen(out_path, "wb");
	Feed<RawChunk> feed(RawProducer{ path, start, stop, batch_bytes, rule == "anywhere" ? CUT_ANYWHERE : CUT_RECORDS });
	while (RawChunk* c = feed.take()) {
		printf("chunk off %llu len %zu last %d\n", (unsigned long long)c->off, c->len, (int)c->last);
		fwrite(c->buf.p, 1, c->len, out);
		const bool last = c->last;
		feed.give_back(c);
		if (last) {
			break;
		}
	}
	fclose(out);
	printf("end error '%s'\n", feed.error().c_str());
	print_allocs();
	return 0;
}

void
print_bgzf(const BgzfChunk& c, FILE* out)
{
	printf("chunk first_member %llu members %zu n_out %llu len %zu last %d whole %d\n", (unsigned long long)c.first_member, c.n_members,
	       (unsigned long long)c.n_out, c.len, (int)c.last, (int)c.whole);
	for (size_t i = 0; i < c.n_members; i++) {
		const ntedit_hip_bgzf_member& m = c.m()[i];
		printf("member in_off %llu out_off %llu n_in %u n_out %u crc %u\n", (unsigned long long)m.in_off, (unsigned long long)m.out_off, m.n_in,
		       m.n_out, m.crc);
	}
	fwrite(c.buf.p, 1, c.len, out);
}

int
run_bgzf(const char* path, size_t batch_bytes, bool thread, const char* out_path)
{
	FILE* out = fopen(out_path, "wb");
	std::string error;
	if (thread) {
		Feed<BgzfChunk> feed(BgzfProducer{ path, batch_bytes });
		while (BgzfChunk* c = feed.take()) {
			print_bgzf(*c, out);
			const bool last = c->last;
			feed.give_back(c);
			if (last) {
				break;
			}
		}
		error = feed.error();
	} else {
		BgzfGather gather(path, batch_bytes);
		BgzfChunk c;
		while (gather.next(&c)) {
			print_bgzf(c, out);
		}
		error = gather.error();
	}
	fclose(out);
	printf("end error '%s'\n", error.c_str());
	return 0;
}

int
run_cut(const char* path, int kind)
{
	std::ifstream in(path, std::ios::binary);
	const std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	for (size_t n = 1; n <= all.size(); n++) {
		char* exact = (char*)malloc(n); // (a block of exactly n bytes: a read past the prefix is reported)
		memcpy(exact, all.data(), n);
		const size_t at = last_record_start(exact, n, kind);
		free(exact);
		printf("%lld\n", at == NO_CUT ? -1ll : (long long)at);
	}
	return 0;
}

} // namespace

int
main(int argc, char** argv)
{
	const std::string cmd = argc > 1 ? argv[1] : "";
	auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
	if (cmd == "queue" && argc >= 3) {
		return run_queue((int)num(2), argc > 3);
	}
	if (cmd == "abandon") {
		return run_abandon();
	}
	if (cmd == "overlap" && argc == 6) {
		return run_overlap(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
	}
	if (cmd == "batch" && argc == 5) {
		return run_batch(argv[2], (unsigned)num(3), (size_t)num(4));
	}
	if (cmd == "raw" && argc == 8) {
		return run_raw(argv[2], num(3), num(4), (size_t)num(5), argv[6], argv[7]);
	}
	if (cmd == "bgzf" && argc == 6) {
		return run_bgzf(argv[2], (size_t)num(3), std::string(argv[4]) == "thread", argv[5]);
	}
	if (cmd == "cut" && argc == 4) {
		return run_cut(argv[2], argv[3][0]);
	}
	fprintf(stderr, "usage: see the head of feed_host.cpp\n");
	return 2;
}
