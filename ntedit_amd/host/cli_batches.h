// cli_batches.h -- the batches of contigs that pass through the three stages of `ntedit` (reader, GPU, writer): their
// buffers, the hand-over queue between the stages and the pool of three that the stages share.  The rules that fill them are
// in batch_rules.h.
#pragma once

#include "../../include/ntedit_hip.h"
#include "batch_rules.h"

#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace nte_cli {

// first touch of a fresh buffer is a page fault per 4 KiB: ask for huge pages on the 2 MiB-aligned part of it
void advise_huge_pages(const void* p, size_t n);

struct Batch
{
	std::string blob; // filled by the streaming reader (append per line) ...
	char* raw = nullptr; // ... or by the mapped reader (whole records copied concurrently; never zero-filled)
	size_t raw_n = 0, raw_cap = 0;
	const char* data() const { return raw_n ? raw : blob.data(); }
	size_t size() const { return raw_n ? raw_n : blob.size(); }
	bool raw_pinned = false; // raw came from ntedit_hip_host_alloc (page-locked: asynchronous H2D at link speed)
	void release_raw();
	bool reserve_raw(size_t n);
	// the batch in the packed form (include/ntedit_hip.h: 4-bit codes + a case bit per base), written by the reader stage:
	// that is what crosses PCIe; the bytes stay for the renderer
	std::vector<char> packed;
	bool is_packed = false;
	std::vector<uint64_t> offs;
	std::vector<uint32_t> lens;
	std::vector<std::string> names;
	std::vector<uint64_t> ordinals; // position of the contig among the contigs >= -z of the whole draft
	void add(uint64_t off, uint32_t len, const std::string& name, uint64_t ordinal)
	{
		offs.push_back(off);
		lens.push_back(len);
		names.push_back(name);
		ordinals.push_back(ordinal);
	}
	void clear();
};

struct Work
{
	Batch b;
	ntedit_hip_result* res = nullptr;
};

// blocking hand-over queue between the pipeline stages (nullptr = end of stream)
class Channel
{
  public:
	void push(Work* w);
	Work* pop();

  private:
	std::mutex mu_;
	std::condition_variable cv_;
	std::deque<Work*> q_;
};

// The three batches of a run.  Their buffers are page-locked (asynchronous H2D at link speed, no staging copies inside the
// polish_batch calls: 0.42 s -> 0.2 s of calls per 3 Gbp), allocated by a side thread WHILE the filter file loads -- i.e.
// before the "reading/processing" stamp, like everything else the reference does before it (ntedit.cpp:2564-2589).  Round 2
// had measured page-locking as a loss because it paid for it inside the timed region, three buffers of 1 GiB.
class BatchPool
{
  public:
	// sizes the buffers for batches of `batch_cap_bases` of the draft at `draft_path` and starts the side thread
	// (`pinned` false: ordinary memory, Batch::reserve_raw allocates on demand)
	BatchPool(int gpu, unsigned long long batch_cap_bases, const std::string& draft_path, bool pinned);
	~BatchPool() { release(); }
	void join_pin_thread();
	void reserve_blobs(size_t bytes); // room for the streaming reader's batches
	void release(); // the buffers go back (before the context that page-locked them is destroyed)
	size_t pin_bytes() const { return pin_bytes_; }
	Work* begin() { return work_; }
	Work* end() { return work_ + 3; }

  private:
	Work work_[3];
	size_t pin_bytes_;
	std::thread pin_thread_;
};

} // namespace nte_cli
