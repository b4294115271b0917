// tile_packed_host.cpp -- the packed tile of nte_tile.h on the CPU: the 1,024 threads of a partition workgroup played one
// after the other, 32 starts each, through tile_stage_packed, tile_prime_packed and the eight-start reader (TileOct) over
// a byte array of the header's LDS size.  For every start the (valid, fh + rh) must equal the BYTE walk's: the same
// positions staged with tile_stage as two byte tiles and walked with TileWalk::roll_bytes.  Test infrastructure only.
//
//   tile_packed_host selftest      prints one line per k and a tally; exit status 0 iff nothing differs
#include "../../ntedit_amd/csrc/nte_tile.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nte;

namespace {

constexpr u32 P_TPB = 1024, P_L = 32; // k_wc_scatter_b's workgroup and starts per thread
static_assert(P_TPB * P_L == (u32)TILE_PACKED_STARTS, "the partition workgroup's tile");

unsigned long long g_starts = 0, g_valid = 0, g_mismatches = 0;

struct Start
{
	bool valid;
	u64 base;
};

struct Lds // s_codes is allocated at exactly TILE_LDS_BYTES so that a sanitizer sees its end
{
	u64 tab[TAB_WORDS];
	u8 lut[256];
	u8* codes;
};

// the byte walk of the TILE_STARTS starts from tile_base
void
byte_tile(Lds& s, const u8* seq, u64 n, u64 tile_base, u32 k, Start* out)
{
	std::memset(s.codes, 0x00, TILE_LDS_BYTES);
	for (u32 tid = 0; tid < (u32)TILE_TPB; tid++) {
		tile_stage(seq, n, tile_base, TILE_STARTS, k, s.lut, s.codes, tid, TILE_TPB);
	}
	for (u32 tid = 0; tid < (u32)TILE_TPB; tid++) {
		const u32 x0 = tid * TILE_L;
		TileWalk w;
		w.prime(s.codes, s.tab, x0, k);
		for (u32 j = 0; j < (u32)TILE_L; j++) {
			out[x0 + j] = Start{ w.valid(), w.base() };
			w.roll_bytes(s.codes, s.tab, j);
		}
	}
}

// the packed walk of the TILE_PACKED_STARTS starts from tile_base, as k_wc_scatter_b stages and reads them
void
packed_tile(Lds& s, const u8* seq, u64 n, u64 tile_base, u32 k, u8 poison, Start* out)
{
	std::memset(s.codes, poison, TILE_LDS_BYTES);
	for (u32 tid = 0; tid < P_TPB; tid++) {
		tile_stage_packed(seq, n, tile_base, TILE_PACKED_STARTS + 8, k, s.lut, s.codes, tid, P_TPB);
	}
	for (u32 tid = 0; tid < P_TPB; tid++) {
		const u32 x0 = tid * P_L;
		TileWalk w;
		tile_prime_packed(w, s.codes, s.tab, x0, k);
		TileOct o;
		o.begin(s.codes, w);
		for (u32 j0 = 0; j0 < P_L; j0 += 8) {
			u32 outw, inw;
			o.read(s.codes, w, j0, outw, inw);
			for (u32 u = 0; u < 8; u++) {
				out[x0 + j0 + u] = Start{ w.valid(), w.base() };
				TileOct::roll(w, s.tab, outw, inw, u);
			}
		}
	}
}

// n bytes of ACGT with N runs, IUPAC codes, lower case and separators planted where a packed tile, its halves (the byte
// tiles), its halo, a thread's stream and a word of eight codes end
u8*
make_batch(u64 n, u32 k, int variant)
{
	void* p = nullptr;
	if (posix_memalign(&p, 16, n ? n : 1) != 0) { // (16-byte aligned as a device batch is, and exactly n bytes long)
		std::abort();
	}
	u8* seq = static_cast<u8*>(p);
	u64 x = 0x9E3779B97F4A7C15ULL * (n + 131 * k + 7);
	for (u64 i = 0; i < n; i++) {
		x = x * 6364136223846793005ULL + 1442695040888963407ULL;
		seq[i] = (u8)"ACGT"[x >> 62];
	}
	const u64 T = TILE_PACKED_STARTS;
	const u64 places[] = { T - 1, T, T + k - 2, T / 2 - 1, T / 2, 2 * T, 5 * 32 + 24, 5 * 32 + 31, 5 * 32 + 24 + k, 5 * 32 + 31 + k,
		                   T + 7 * 32 + 29 + k, 777, 778, 64 * 32 - 1, 64 * 32 };
	const u8 odd[5] = { 'N', 'R', 'g', '\n', 'Y' };
	for (size_t i = 0; i < sizeof places / sizeof places[0]; i++) {
		if (places[i] < n) {
			seq[places[i]] = odd[(i + (size_t)variant) % 5];
		}
	}
	// an N run across the middle of a packed tile (the byte tiles' boundary) and a separator between two short contigs
	for (u64 i = T / 2 - 7; i < T / 2 + 8 && i < n; i++) {
		seq[i] = 'N';
	}
	if (n > 3000) {
		seq[2000] = '\n';
		seq[2000 + (k > 1 ? k - 1 : 1)] = '\n'; // a contig of k - 2 bases: no k-mer
	}
	return seq;
}

void
check_batch(Lds& s, const u64* tabs, u32 k, u64 n, int variant)
{
	u8* seq = make_batch(n, k, variant);
	const u64 T = TILE_PACKED_STARTS;
	const u64 tiles = n ? (n + T - 1) / T : 1;
	std::vector<Start> want(T), a(T), b(T);
	for (int rule = 0; rule < 2; rule++) {
		for (u32 tid = 0; tid < (u32)TILE_TPB; tid++) {
			tile_load_tabs(tabs, s.tab, tid);
			tile_fill_lut(s.lut, rule == 1, tid);
		}
		for (u64 tile = 0; tile < tiles; tile++) {
			byte_tile(s, seq, n, tile * T, k, want.data());
			byte_tile(s, seq, n, tile * T + TILE_STARTS, k, want.data() + TILE_STARTS);
			packed_tile(s, seq, n, tile * T, k, 0x00, a.data());  // poison: two codes of an A
			packed_tile(s, seq, n, tile * T, k, 0xFF, b.data());  // poison: two codes that end a k-mer
			for (u32 j = 0; j < (u32)T; j++) {
				const Start* got[2] = { &a[j], &b[j] };
				for (int g = 0; g < 2; g++) {
					if (got[g]->valid != want[j].valid || got[g]->base != want[j].base) {
						if (g_mismatches++ < 20) {
							std::printf("MISMATCH eight-start reader%s: k %u n %llu lut %d start %llu\n", g ? ", second poison" : "", k,
							            (unsigned long long)n, rule, (unsigned long long)(tile * T + j));
						}
					}
				}
				g_starts++;
				g_valid += want[j].valid;
			}
		}
	}
	std::free(seq);
}

int
selftest()
{
	Lds s;
	s.codes = static_cast<u8*>(std::malloc(TILE_LDS_BYTES));
	if (!s.codes) {
		return 2;
	}
	const u32 ks[] = { 1, 7, 8, 9, 25, 31, 32, 33, 255, 256 };
	for (u32 k : ks) {
		u64 tabs[TAB_WORDS];
		build_seed_tables(k, tabs);
		const unsigned long long starts0 = g_starts, valid0 = g_valid, mis0 = g_mismatches;
		const u64 T = TILE_PACKED_STARTS;
		// shorter than k, exactly k, bytes past the batch end inside a tile, whole tiles, a halo that ends with the batch
		const u64 ns[] = { k - 1, k, T - 17, T, T + k - 1, 2 * T + 5 };
		for (u64 n : ns) {
			check_batch(s, tabs, k, n, 0);
		}
		for (int variant = 1; variant < 5; variant++) {
			check_batch(s, tabs, k, T + k + 3, variant);
		}
		std::printf("k %u: starts %llu valid %llu mismatches %llu\n", k, g_starts - starts0, g_valid - valid0, g_mismatches - mis0);
	}
	std::free(s.codes);
	std::printf("starts %llu valid %llu mismatches %llu\n", g_starts, g_valid, g_mismatches);
	return g_mismatches ? 1 : 0;
}

} // namespace

int
main(int argc, char** argv)
{
	if (argc == 2 && std::strcmp(argv[1], "selftest") == 0) {
		return selftest();
	}
	std::fprintf(stderr, "usage: tile_packed_host selftest\n");
	return 2;
}
