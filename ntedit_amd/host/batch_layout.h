// batch_layout.h -- the layout rule of a batch: n bytes that hold the entries [offs[i], offs[i] + lens[i]) in order.  Host only,
// no I/O and no library call (the library's entry points check their arguments with it; the CPU tests compile it on its own).
#pragma once

#include <cstdint>

namespace nte_host {

constexpr uint32_t LAYOUT_OK = 0xFFFFFFFFu;

// The index of the first entry that breaks the layout, or LAYOUT_OK: an entry lies inside the n bytes and ends at or before
// the start of the next one -- before it when `separated` (the polish: at least one byte between two entries), while the
// other callers take entries that abut.  No sum is formed before both of its terms are known to lie within n.
inline uint32_t
first_layout_break(uint64_t n, const uint64_t* offs, const uint32_t* lens, uint32_t n_entries, bool separated)
{
	for (uint32_t i = 0; i < n_entries; i++) {
		if (offs[i] > n || lens[i] > n - offs[i]) {
			return i;
		}
		const uint64_t end = offs[i] + lens[i]; // (<= n)
		if (i + 1 < n_entries && (separated ? end >= offs[i + 1] : end > offs[i + 1])) {
			return i;
		}
	}
	return LAYOUT_OK;
}

} // namespace nte_host
