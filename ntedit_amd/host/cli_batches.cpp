// cli_batches.cpp -- see cli_batches.h
#include "cli_batches.h"

#include <cstdio>
#include <cstdlib>
#include <sys/mman.h>
#include <sys/stat.h>

namespace nte_cli {

void
advise_huge_pages(const void* p, size_t n)
{
	const uintptr_t lo = ((uintptr_t)p + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1);
	const uintptr_t hi = ((uintptr_t)p + n) & ~(uintptr_t)((2u << 20) - 1);
	if (hi > lo) {
		(void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
	}
}

void
Batch::release_raw()
{
	if (raw_pinned) {
		ntedit_hip_host_free(raw);
	} else {
		free(raw);
	}
	raw = nullptr;
	raw_cap = 0;
	raw_pinned = false;
}

bool
Batch::reserve_raw(size_t n)
{
	if (n > raw_cap) {
		release_raw();
		raw_cap = n + n / 8 + (1u << 20);
		raw = (char*)malloc(raw_cap);
		if (raw) {
			advise_huge_pages(raw, raw_cap);
		} else {
			raw_cap = 0;
		}
	}
	return raw != nullptr;
}

void
Batch::clear()
{
	blob.clear();
	raw_n = 0;
	is_packed = false;
	offs.clear();
	lens.clear();
	names.clear();
	ordinals.clear();
}

void
Channel::push(Work* w)
{
	{
		std::lock_guard<std::mutex> lk(mu_);
		q_.push_back(w);
	}
	cv_.notify_one();
}

Work*
Channel::pop()
{
	std::unique_lock<std::mutex> lk(mu_);
	cv_.wait(lk, [&]() { return !q_.empty(); });
	Work* w = q_.front();
	q_.pop_front();
	return w;
}

//  a small draft does not pay for the largest batch: a plain FASTA file holds no more bases than it has bytes
// (3 x 1 GiB of page-locked memory and ~30 GB of device buffers for a 5 Mbp draft otherwise).  Compressed drafts keep the
// full size: their length is not known in advance.
static size_t
buffer_bytes(unsigned long long batch_cap_bases, const std::string& draft_path)
{
	size_t bytes = (size_t)(batch_cap_bases < (1ull << 32) ? batch_cap_bases : (1ull << 32)) + (size_t)(64u << 20);
	struct stat sb;
	FILE* probe = fopen(draft_path.c_str(), "rb");
	if (probe) {
		unsigned char magic[2] = { 0, 0 };
		const bool gz = fread(magic, 1, 2, probe) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
		if (!gz && fstat(fileno(probe), &sb) == 0 && S_ISREG(sb.st_mode)) {
			const size_t by_file = (size_t)sb.st_size + (size_t)(4u << 20);
			if (by_file < bytes) {
				bytes = by_file;
			}
		}
		fclose(probe);
	}
	return bytes;
}

BatchPool::BatchPool(int gpu, unsigned long long batch_cap_bases, const std::string& draft_path, bool pinned)
  : pin_bytes_(buffer_bytes(batch_cap_bases, draft_path))
{
	pin_thread_ = std::thread([this, gpu, pinned]() {
		(void)ntedit_hip_bind_near_device(gpu);
		if (!pinned) {
			return;
		}
		for (Work& w : *this) {
			char* m = (char*)ntedit_hip_host_alloc(pin_bytes_);
			if (!m) {
				return; // (ordinary memory then: reserve_raw allocates on demand)
			}
			w.b.raw = m;
			w.b.raw_cap = pin_bytes_;
			w.b.raw_pinned = true;
		}
	});
}

void
BatchPool::reserve_blobs(size_t bytes)
{
	for (Work& w : *this) {
		w.b.blob.reserve(bytes); // (address space only: pages are touched as the batch fills)
		advise_huge_pages(w.b.blob.data(), w.b.blob.capacity());
	}
}

void
BatchPool::join_pin_thread()
{
	if (pin_thread_.joinable()) {
		pin_thread_.join();
	}
}

void
BatchPool::release()
{
	join_pin_thread();
	for (Work& w : *this) {
		w.b.release_raw();
	}
}

} // namespace nte_cli
