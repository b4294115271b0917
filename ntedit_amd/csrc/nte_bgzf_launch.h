// nte_bgzf_launch.h -- the BGZF writer on the device (nte_bgzf_deflate.hip): what nte_api.hip calls.
//
// The unit sees no context internals: its state hangs off the `owner` pointer, its device buffers grow only and go with
// bgzf_release (ntedit_hip_destroy).  Every call works on the stream it is given and leaves it drained.  Stages:
//   k_fa_image     the _edited.fa text of a batch from the applier's output: '>' name '\n', then the entry's bytes and its
//                  separator byte, entry after entry; workgroup per tile of 16 KiB of the image
//   k_bz_deflate   wavefront per block of 65,280 image bytes, into that block's 64 KiB slot; the member's size per block
//   k_bz_scan      one workgroup: the exclusive 64-bit scan of the sizes, the stored members counted
//   k_bz_pack      workgroup per member: its bytes from the slot to its scanned offset, the members contiguous
#pragma once
#include "nte_common.h"

#include <hip/hip_runtime.h>

#include <string>

namespace nte {

struct BgzfTotals
{
	u64 plain = 0, bytes = 0;
	u32 members = 0, stored = 0;
	float ms_image = 0.f, ms_deflate = 0.f, ms_copy = 0.f;
};

// a batch's entries as the applier left them (host tables, device bytes) and their header lines
struct FaImage
{
	const u8* d_edited;
	const u64* e_offs; // host, n
	const u32* e_lens; // host, n
	u32 n;
	const char* names;    // host: the names' bytes, one behind the other
	const u64* name_offs; // host, n + 1
};

// 0, or an NTEDIT_E_* code with *why set
int bgzf_image(const void* owner, int device, hipStream_t s, const FaImage& im, const u8** d_image, u64* n_image, float* ms, std::string* why);
// src (device bytes) in blocks of 65,280 into packed members in the unit's buffer; t: plain, bytes, members, stored, ms_deflate
int bgzf_encode(const void* owner, int device, hipStream_t s, const u8* d_src, u64 n, BgzfTotals* t, std::string* why);
// the packed members of the last bgzf_encode to host memory
int bgzf_fetch(const void* owner, hipStream_t s, void* host_dst, u64 bytes, float* ms_copy, std::string* why);
// host bytes to the unit's own source buffer (the stand-alone call on host bytes)
int bgzf_upload(const void* owner, int device, hipStream_t s, const void* host_src, u64 n, const u8** d_src, std::string* why);
// buffers for images of up to max_image bytes, and one small block through every kernel
int bgzf_reserve(const void* owner, int device, hipStream_t s, u64 max_image, u32 max_entries, std::string* why);
void bgzf_release(const void* owner);

} // namespace nte
