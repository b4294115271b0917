// bgzf_walk.h -- the member walk of BGZF (the SAM specification, section 4.1), as FastaMap::inflate_bgzf walks it: gzip
// members with FLG = FEXTRA and an extra subfield 'B','C' of two bytes holding the member's total size - 1; CRC-32 and
// ISIZE close each member.  Host code without a dependency: ntedit_hip_bgzf_walk (nte_reads_inflate.hip) is this behind
// an argument check, and the chunk feeders (chunk_feed.h) call it directly, so they build without the library.
#pragma once

#include "../../include/ntedit_hip.h"

#include <cstdint>
#include <cstring>

namespace nte_host {

inline uint32_t
le16(const unsigned char* d)
{
	return (uint32_t)d[0] | (uint32_t)d[1] << 8;
}

inline uint32_t
le32(const unsigned char* d)
{
	return le16(d) | le16(d + 2) << 16;
}

inline int
bgzf_walk(const void* bytes, uint64_t n, ntedit_hip_bgzf_member* members, uint64_t cap, uint64_t* n_members, uint64_t* consumed)
{
	const unsigned char* d = (const unsigned char*)bytes;
	uint64_t o = 0, count = 0, total = 0;
	int rc = NTEDIT_BGZF_END;
	while (o < n) {
		static const unsigned char magic[4] = { 0x1f, 0x8b, 8, 4 };
		const uint64_t left = n - o;
		if (memcmp(d + o, magic, left < 4 ? left : 4) != 0) {
			rc = NTEDIT_BGZF_NOT;
			break;
		}
		if (left < 12) {
			rc = NTEDIT_BGZF_CUT;
			break;
		}
		const uint32_t xlen = le16(d + o + 10);
		if (left < 12 + (uint64_t)xlen) {
			rc = NTEDIT_BGZF_CUT;
			break;
		}
		uint32_t bsize = 0;
		bool have = false;
		for (uint64_t x = o + 12; x + 4 <= o + 12 + xlen;) {
			const uint32_t slen = le16(d + x + 2);
			if (d[x] == 'B' && d[x + 1] == 'C' && slen == 2 && x + 6 <= o + 12 + xlen) {
				bsize = le16(d + x + 4);
				have = true;
			}
			x += 4 + (uint64_t)slen;
		}
		const uint64_t member = (uint64_t)bsize + 1;
		if (!have || member < 12 + (uint64_t)xlen + 8) {
			rc = NTEDIT_BGZF_NOT;
			break;
		}
		if (member > left) {
			rc = NTEDIT_BGZF_CUT;
			break;
		}
		const uint32_t n_out = le32(d + o + member - 4);
		if (n_out > 65536) {
			rc = NTEDIT_BGZF_NOT;
			break;
		}
		if (count == cap) {
			rc = NTEDIT_BGZF_FULL;
			break;
		}
		ntedit_hip_bgzf_member& m = members[count++];
		m.in_off = o + 12 + xlen;
		m.out_off = total;
		m.n_in = (uint32_t)(member - 12 - xlen - 8);
		m.n_out = n_out;
		m.crc = le32(d + o + member - 8);
		m.reserved = 0;
		total += n_out;
		o += member;
	}
	*n_members = count;
	*consumed = o;
	return rc;
}

} // namespace nte_host
