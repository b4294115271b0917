// deflate_host.cpp -- TEST-ONLY: the encoder of ntedit_amd/csrc/nte_bgzf_deflate.h on the CPU, one lane, the way the
// library's serial model runs it, over a file of cases; every member it writes is decoded twice, by zlib's inflate and
// by the project's own decoder (nte_bgzf_inflate.h), and compared with the block it was made from.  Built plain and
// with -fsanitize=address,undefined (tests/test_bgzf_deflate_cpu.py): every block is a heap block of its exact size, the
// slot a heap block of exactly DZ_SLOT bytes.
//
//   deflate_host CASES [OUT]    CASES: u32 count, then per case u32 length and the bytes.  OUT: the members of all cases,
//                               one behind the other (the test compares them with the library model's)
// Last line: "cases N members M stored S bytes B mismatches X".
#include "nte_bgzf_deflate.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nte_bgzf;

static uint32_t
le32(const uint8_t* p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the member against the block: the header's fields, the trailer, the payload through both decoders
static bool
member_ok(const uint8_t* m, uint32_t size, const uint8_t* block, uint32_t n, uint32_t stored, BzTables* bt)
{
	if (size < DZ_HEAD + DZ_TAIL + 1 || size > DZ_SLOT) {
		return false;
	}
	static const uint8_t head[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
	if (memcmp(m, head, 16) != 0 || (uint32_t)(m[16] | m[17] << 8) != size - 1) {
		return false;
	}
	if (le32(m + size - 4) != n || le32(m + size - 8) != (uint32_t)crc32(crc32(0, nullptr, 0), block, n)) {
		return false;
	}
	if (stored != ((m[DZ_HEAD] & 7) == 1 ? 1u : 0u) || (stored && size != DZ_HEAD + DZ_STORED + n + DZ_TAIL)) {
		return false;
	}
	const uint32_t n_in = size - DZ_HEAD - DZ_TAIL;
	// zlib: raw inflate of the payload, which must end exactly at the trailer
	uint8_t* a = (uint8_t*)malloc(n);
	z_stream z;
	memset(&z, 0, sizeof z);
	bool ok = inflateInit2(&z, -15) == Z_OK;
	if (ok) {
		z.next_in = const_cast<uint8_t*>(m) + DZ_HEAD;
		z.avail_in = n_in;
		z.next_out = a;
		z.avail_out = n;
		ok = inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_in == 0 && z.avail_out == 0 && memcmp(a, block, n) == 0;
		inflateEnd(&z);
	}
	free(a);
	// the project's decoder, on heap copies of the exact sizes
	uint8_t* in = (uint8_t*)malloc(n_in);
	uint8_t* b = (uint8_t*)malloc(n);
	memcpy(in, m + DZ_HEAD, n_in);
	ok = bz_inflate(in, n_in, b, n, bt, 0, 1) == BZ_OK && memcmp(b, block, n) == 0 && ok;
	free(in);
	free(b);
	return ok;
}

int
main(int argc, char** argv)
{
	if (argc < 2) {
		fprintf(stderr, "usage: deflate_host CASES [OUT]\n");
		return 2;
	}
	FILE* f = fopen(argv[1], "rb");
	FILE* o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
	uint32_t count = 0;
	if (!f || (argc > 2 && !o) || fread(&count, 4, 1, f) != 1) {
		fprintf(stderr, "deflate_host: cannot open the files\n");
		return 2;
	}
	DzTables* t = new DzTables();
	BzTables* bt = new BzTables();
	unsigned long long members = 0, n_stored = 0, bytes = 0, mismatches = 0;
	for (uint32_t c = 0; c < count; c++) {
		uint32_t len = 0;
		if (fread(&len, 4, 1, f) != 1) {
			return 2;
		}
		std::vector<uint8_t> data(len);
		if (len && fread(data.data(), 1, len, f) != len) {
			return 2;
		}
		for (uint64_t at = 0; at < len; at += DZ_BLOCK) {
			const uint32_t n = len - at < DZ_BLOCK ? (uint32_t)(len - at) : DZ_BLOCK;
			uint8_t* block = (uint8_t*)malloc(n);
			uint8_t* slot = (uint8_t*)malloc(DZ_SLOT);
			memcpy(block, data.data() + at, n);
			memset(slot, 0xEE, DZ_SLOT);
			uint32_t stored = 0;
			const uint32_t size = dz_member(block, n, slot, t, 0, 1, &stored);
			if (!member_ok(slot, size, block, n, stored, bt)) {
				mismatches++;
				printf("case %u block at %llu (%u bytes): the member does not give the block back\n", c, (unsigned long long)at, n);
			}
			if (o && size <= DZ_SLOT) {
				fwrite(slot, 1, size, o);
			}
			members++;
			n_stored += stored;
			bytes += size;
			free(slot);
			free(block);
		}
	}
	delete t;
	delete bt;
	fclose(f);
	if (o && fclose(o) != 0) {
		return 2;
	}
	printf("cases %u members %llu stored %llu bytes %llu mismatches %llu\n", count, members, n_stored, bytes, mismatches);
	return mismatches ? 1 : 0;
}
