// batch_rules.h -- which contigs of the draft a run polishes and where its batches are cut.  Host only, no I/O and no
// library call (cli_batches.h; the CPU tests compile it on its own).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace nte_cli {

// --shard I/N: the contigs >= -z, given by their lengths in draft order, split by bases, greedy longest-first (the partition
// of ntedit_amd.dist.shard_contigs).  Returns, by ordinal, whether the contig is share shard_i's.
inline std::vector<uint8_t>
shard_partition(const std::vector<uint64_t>& lens, unsigned shard_n, unsigned shard_i)
{
	std::vector<uint32_t> order(lens.size());
	for (size_t i = 0; i < order.size(); i++) {
		order[i] = (uint32_t)i;
	}
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
	std::vector<uint64_t> load(shard_n, 0);
	std::vector<uint8_t> mine(lens.size(), 0);
	for (uint32_t i : order) {
		unsigned best = 0;
		for (unsigned r = 1; r < shard_n; r++) {
			if (load[r] < load[best]) {
				best = r;
			}
		}
		load[best] += lens[i];
		mine[i] = best == shard_i;
	}
	return mine;
}

// The admission rule of the draft readers: offered the contigs of the draft in order, by length, it answers whether the run
// skips a contig, takes it into the open batch, or closes that batch and takes it as the first of the next.  A batch holds
// each contig's bases and one byte more; it is closed when the next contig would take it over the budget, so the first contig
// of a batch always fits and no batch is empty.  The budget doubles with every batch closed, up to `cap`.
class Admission
{
  public:
	enum Verdict
	{
		SKIP,
		TAKE,
		CLOSE_THEN_TAKE,
		TOO_LONG // a contig of the run is longer than 2^32 bases: an error
	};

	// `mine`: by ordinal, the contigs of this shard (nullptr: all of them)
	Admission(uint64_t min_len, const std::vector<uint8_t>* mine, uint64_t budget, uint64_t cap)
	  : min_len_(min_len)
	  , mine_(mine)
	  , budget_(budget)
	  , cap_(cap)
	{}

	Verdict offer(uint64_t len)
	{
		seen_++;
		if (len < min_len_) { // ntedit.cpp:2242
			return SKIP;
		}
		const uint64_t ordinal = next_ordinal_++;
		if (mine_ && !(ordinal < mine_->size() && (*mine_)[ordinal])) {
			return SKIP;
		}
		if (len > 0xFFFFFFF0ull) {
			return TOO_LONG;
		}
		const bool full = count_ != 0 && total_ + len + 1 > budget_;
		if (full) {
			budget_ = budget_ * 2 < cap_ ? budget_ * 2 : cap_;
			total_ = 0;
			count_ = 0;
		}
		ordinal_ = ordinal;
		offset_ = total_;
		total_ += len + 1;
		count_++;
		bases_ += len;
		return full ? CLOSE_THEN_TAKE : TAKE;
	}

	// of the contig taken last: its position among the contigs >= -z of the whole draft, and its offset in its batch
	uint64_t ordinal() const { return ordinal_; }
	uint64_t offset() const { return offset_; }
	uint64_t seen() const { return seen_; }     // contigs offered
	uint64_t bases() const { return bases_; }   // bases taken
	uint64_t budget() const { return budget_; } // of the open batch

  private:
	uint64_t min_len_;
	const std::vector<uint8_t>* mine_;
	uint64_t budget_, cap_;
	uint64_t seen_ = 0, next_ordinal_ = 0, ordinal_ = 0, offset_ = 0, total_ = 0, count_ = 0, bases_ = 0;
};

} // namespace nte_cli
