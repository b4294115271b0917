// nte_reads_unit.h -- what the three device units of the reads front end (nte_reads_parse.hip, nte_reads_inflate.hip,
// nte_reads_bam.hip) are built alike from, written once: a unit's per-context state and its registry, the carver of one
// allocation into aligned parts, and (HIP sources only) the error macro and the grow-only device buffer.
//
// A unit sees no context internals: its state hangs off the context pointer.  The state is two structs: Keep is what the
// calls set and the last pass counted, and survives ntedit_hip_sketch_free; Scratch is the device, events and buffers,
// which a unit's release function frees and then resets with `scr = Scratch()`.  A field is in one or the other, so
// nothing is saved and restored by hand.
//
// The first part needs no HIP and compiles under a plain host compiler (tests/unit/unit_host.cpp), as nte_tile.h does.
#pragma once

#include <stdint.h>

#include <deque>
#include <mutex>

namespace nte_unit {

inline uint64_t
up256(uint64_t x)
{
	return (x + 255) / 256 * 256;
}

// one allocation cut into parts that each start at a multiple of 256 bytes; a null base only adds up the sizes
struct Carver
{
	uint8_t* base;
	uint64_t at = 0; // the bytes taken so far: the allocation's size once every part is taken

	explicit Carver(uint8_t* b) : base(b) {}

	uint8_t* take(uint64_t bytes)
	{
		uint8_t* p = base ? base + at : nullptr;
		at += up256(bytes);
		return p;
	}
};

template<class Keep, class Scratch>
struct State
{
	const void* owner = nullptr; // the context
	Keep keep;
	Scratch scr;
};

// the states of one unit, one per context that called it, found by the context pointer; a state lives as long as the registry
template<class S>
class Registry
{
public:
	S* find(const void* owner, bool create)
	{
		std::lock_guard<std::mutex> lk(mu_);
		for (S& s : all_) {
			if (s.owner == owner) {
				return &s;
			}
		}
		if (!create) {
			return nullptr;
		}
		all_.emplace_back();
		all_.back().owner = owner;
		return &all_.back();
	}

	size_t size()
	{
		std::lock_guard<std::mutex> lk(mu_);
		return all_.size();
	}

private:
	std::mutex mu_;
	std::deque<S> all_; // (a deque: a state's address holds while others are added)
};

} // namespace nte_unit

#if defined(__HIP__) || defined(__HIPCC__)
#include "nte_reads_internal.h"

#include <hip/hip_runtime.h>

#include <string>

namespace nte_unit {

// a unit's failures go to the store of ntedit_hip_reads_last_error (nte_reads.hip)
inline int
pfail(const ntedit_hip_ctx* c, int code, const std::string& why)
{
	return nte_reads::set_error(c, code, why);
}

#define NTE_TRY(ctx, expr)                                                                                  \
	do {                                                                                                    \
		hipError_t e_ = (expr);                                                                             \
		if (e_ != hipSuccess) {                                                                             \
			return nte_unit::pfail((ctx), NTEDIT_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
		}                                                                                                   \
	} while (0)

// a grow-only device buffer: cap is what its unit may use of it
struct DevBuf
{
	uint8_t* p = nullptr;
	uint64_t cap = 0;
};

// buf to at least `need` bytes.  When it is too small it is replaced by one of `want` bytes (the unit's sizing rule; `behind`
// more are allocated and not counted in cap).  A buffer in use is freed only after `stream`, which works on it, is
// drained; its first `keep` bytes are copied to the new one first, on that stream.
inline int
grow(const ntedit_hip_ctx* c, hipStream_t stream, DevBuf* buf, uint64_t need, uint64_t want, uint64_t keep = 0, uint64_t behind = 0)
{
	if (need <= buf->cap && buf->p) {
		return 0;
	}
	uint8_t* q = nullptr;
	if (buf->p && keep) {
		NTE_TRY(c, hipMalloc((void**)&q, want + behind));
		NTE_TRY(c, hipMemcpyAsync(q, buf->p, keep, hipMemcpyDeviceToDevice, stream));
	}
	if (buf->p) {
		NTE_TRY(c, hipStreamSynchronize(stream));
		NTE_TRY(c, hipFree(buf->p));
		*buf = DevBuf();
	}
	if (!q) {
		NTE_TRY(c, hipMalloc((void**)&q, want + behind));
	}
	buf->p = q;
	buf->cap = want;
	return 0;
}

} // namespace nte_unit
#endif
