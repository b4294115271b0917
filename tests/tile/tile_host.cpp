// tile_host.cpp -- nte_tile.h on the CPU: the 256 threads of a workgroup played one after the other over a byte array of
// the header's LDS size.  Every tile is staged first, then walked with both reader forms; for every start both must give
// the (valid, fh + rh) of a direct computation: a fresh HashState rolled over exactly those k codes, and "all k codes
// good".  Then the entry cursor against a linear scan, entry_behind and byte_sat_inc.  Test infrastructure only.
//
//   tile_host selftest      prints one line per k and a tally; exit status 0 iff nothing differs
#include "../../ntedit_amd/csrc/nte_tile.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nte;

namespace {

unsigned long long g_starts = 0, g_valid = 0, g_mismatches = 0;

void
mismatch(const char* what, u32 k, u64 n, int rule, u64 pos)
{
	if (g_mismatches++ < 20) {
		std::printf("MISMATCH %s: k %u n %llu lut %d start %llu\n", what, k, (unsigned long long)n, rule, (unsigned long long)pos);
	}
}

// the code of position pos of a batch of n bytes under a look-up rule, restated: past n a '\n'
u8
code_at(const u8* seq, u64 n, u64 pos, bool acgt_only)
{
	const u8 code = char_code(pos < n ? seq[pos] : (u8)'\n');
	return acgt_only && code > 3 ? CODE_BAD : code;
}

struct Start
{
	bool valid;
	u64 base;
};

struct Lds // what a workgroup holds; s_codes is allocated at exactly TILE_LDS_BYTES so that a sanitizer sees its end
{
	u64 tab[TAB_WORDS];
	u8 lut[256];
	u8* codes;
};

// one tile through the header, both reader forms; bytes[] and quads[] get TILE_STARTS results each
void
run_tile(Lds& s, const u8* seq, u64 n, u64 tile, u32 k, u8 poison, Start* bytes, Start* quads)
{
	std::memset(s.codes, poison, TILE_LDS_BYTES);
	for (u32 tid = 0; tid < (u32)TILE_TPB; tid++) {
		tile_stage(seq, n, tile * TILE_STARTS, TILE_STARTS, k, s.lut, s.codes, tid, TILE_TPB);
	}
	for (u32 tid = 0; tid < (u32)TILE_TPB; tid++) {
		const u32 x0 = tid * TILE_L;
		TileWalk w;
		w.prime(s.codes, s.tab, x0, k);
		for (u32 j = 0; j < (u32)TILE_L; j++) {
			bytes[x0 + j] = Start{ w.valid(), w.base() };
			w.roll_bytes(s.codes, s.tab, j);
		}
		TileWalk v;
		v.prime(s.codes, s.tab, x0, k);
		TileQuad q;
		q.begin(s.codes, v);
		for (u32 j0 = 0; j0 < (u32)TILE_L; j0 += 4) {
			u32 outw, inw;
			q.read(s.codes, v, j0, outw, inw);
			for (int u = 0; u < 4; u++) {
				quads[x0 + j0 + u] = Start{ v.valid(), v.base() };
				v.roll_quad(s.tab, outw, inw, u);
			}
		}
	}
}

// a batch of n bytes of ACGT with the odd bytes planted: N, an IUPAC R, lower case and '\n', rotated by `variant` over
// the places where a tile, its halo and a stream end
std::vector<u64>
planted_places(u32 k)
{
	const u64 T = TILE_STARTS;
	return { T - 1, T,              // 16383 and 16384 (the first halo byte of tile 0)
		     T + k - 2,             // the last halo byte of tile 0
		     2 * T,                 // the first halo byte of tile 1
		     3 * 64 + 60, 3 * 64 + 63,         // the last word of four a stream rolls out
		     3 * 64 + 60 + k, 3 * 64 + 63 + k, // ... and rolls in
		     T + 5 * 64 + 61 + k, 777 };
}

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
	const u8 odd[4] = { 'N', 'R', 'g', '\n' };
	const std::vector<u64> places = planted_places(k);
	for (size_t i = 0; i < places.size(); i++) {
		if (places[i] < n) {
			seq[places[i]] = odd[(i + (size_t)variant) & 3];
		}
	}
	return seq;
}

void
check_batch(Lds& s, const u64* tabs, u32 k, u64 n, int variant)
{
	u8* seq = make_batch(n, k, variant);
	const u64 tiles = n ? (n + TILE_STARTS - 1) / TILE_STARTS : 1; // (an empty batch: one tile all the same)
	std::vector<Start> a(TILE_STARTS), b(TILE_STARTS), a2(TILE_STARTS), b2(TILE_STARTS);
	for (int rule = 0; rule < 2; rule++) {
		const bool acgt_only = rule == 1;
		for (u32 tid = 0; tid < (u32)TILE_TPB; tid++) {
			tile_load_tabs(tabs, s.tab, tid);
			tile_fill_lut(s.lut, acgt_only, tid);
		}
		for (u64 tile = 0; tile < tiles; tile++) {
			// (a poison is a code: with k = 1 mod 16 a stream's last roll, whose state nobody reads, takes in the byte behind
			// what was staged, and k = 256 reads a word there)
			run_tile(s, seq, n, tile, k, 0x00, a.data(), b.data());     // poison: the code of an A
			run_tile(s, seq, n, tile, k, CODE_BAD, a2.data(), b2.data()); // poison: the code that ends a k-mer
			const u64 p0 = tile * TILE_STARTS;
			for (u32 j = 0; j < (u32)TILE_STARTS; j++) {
				const u64 pos = p0 + j;
				bool all_good = true;
				HashState hs = { 0, 0 };
				for (u32 i = 0; i < k; i++) {
					const u8 c = code_at(seq, n, pos + i, acgt_only);
					all_good = all_good && c != CODE_BAD;
					hash_roll(hs, tabs, CODE_BAD, c);
				}
				const Start want = { all_good, hs.fh + hs.rh };
				const Start* got[4] = { &a[j], &b[j], &a2[j], &b2[j] };
				static const char* const names[4] = { "byte reader", "four-start reader", "byte reader, second poison", "four-start reader, second poison" };
				for (int g = 0; g < 4; g++) {
					if (got[g]->valid != want.valid || got[g]->base != want.base) {
						mismatch(names[g], k, n, rule, pos);
					}
				}
				g_starts++;
				g_valid += want.valid;
			}
		}
	}
	std::free(seq);
}

// ---------------------------------------------------------------- the entries
void
check_entries(u32 k)
{
	const u64 T = TILE_STARTS;
	std::vector<u64> offs;
	std::vector<u32> lens;
	auto add = [&](u64 o, u64 len) {
		offs.push_back(o);
		lens.push_back((u32)len);
	};
	add(0, 100);
	add(100, k - 1);          // abuts, shorter than k
	add(100 + k - 1, 0);      // abuts, empty
	add(100 + k - 1, k);      // abuts, exactly k
	add(100 + 2 * k - 1, T - (100 + 2 * k - 1)); // abuts, ends exactly at 16384
	add(T + 16, k);           // behind a gap
	add(T + 16 + k + 5, 0);   // empty, in a gap
	add(T + 1000, 300);
	add(T + 1300, 3 * k + 1); // abuts; the last entry: every position behind T + 1300 + 3k + 1 lies behind all entries
	const u32 n_entries = (u32)offs.size();
	auto scan = [&](u64 x) { // the definition: the first entry whose end lies behind x
		u32 e = 0;
		while (e < n_entries && offs[e] + lens[e] <= x) {
			e++;
		}
		return e;
	};
	u64 inside = 0;
	const u32 counts[3] = { 0, 1, n_entries };
	for (u32 ne : counts) {
		for (u64 x = 0; x < 2 * T; x += (x < 300 || (x > T - 50 && x < T + 1800)) ? 1 : 97) {
			u32 want = 0;
			while (want < ne && offs[want] + lens[want] <= x) {
				want++;
			}
			if (entry_behind(offs.data(), lens.data(), ne, x) != want) {
				mismatch("entry_behind", k, x, (int)ne, x);
			}
		}
	}
	for (u32 tid = 0; tid < 2 * (u32)TILE_TPB; tid++) { // two tiles of streams, the second mostly behind the last entry
		const u64 pos0 = (u64)tid * TILE_L;
		EntryCursor cur;
		cur.start(offs.data(), lens.data(), n_entries, pos0);
		for (u32 j = 0; j < (u32)TILE_L; j++) {
			const u64 pos = pos0 + j;
			cur.advance(offs.data(), lens.data(), n_entries, pos);
			const u32 e = scan(pos);
			const u64 eb = e < n_entries ? offs[e] : ~0ULL, ee = e < n_entries ? offs[e] + lens[e] : ~0ULL;
			const bool holds = e < n_entries && pos >= offs[e] && pos + k <= offs[e] + lens[e];
			if (cur.e != e || cur.eb != eb || cur.ee != ee || cur.holds(pos, k) != holds) {
				mismatch("entry cursor", k, 0, 0, pos);
			}
			inside += holds;
		}
	}
	// what lies inside an entry: every entry of at least k bytes has len - k + 1 starts
	u64 want_inside = 0;
	for (u32 e = 0; e < n_entries; e++) {
		want_inside += lens[e] >= k ? lens[e] - k + 1 : 0;
	}
	if (inside != want_inside) {
		mismatch("starts inside entries", k, inside, 0, want_inside);
	}
}

void
check_bit_range()
{
	for (u32 lo = 0; lo <= 64; lo++) {
		for (u32 hi = 0; hi <= 64; hi++) {
			u64 want = 0;
			for (u32 b = lo; b < hi; b++) {
				want |= 1ULL << b;
			}
			if (bit_range(lo, hi) != want) {
				mismatch("bit_range", lo, hi, 0, 0);
			}
		}
	}
}

void
check_byte_sat_inc()
{
	for (u32 b = 0; b < 4; b++) {
		u32 words[3] = { 0xFFFEFDFCu, 0x7FFEFF00u, 0x00FFFEFDu };
		const u32 before[3] = { words[0], words[1], words[2] };
		const u32 sh = 8 * b;
		u32 v = (before[1] >> sh) & 0xFF;
		for (int i = 0; i < 300; i++) {
			byte_sat_inc(words, 4 + b);
			v = v < 255 ? v + 1 : 255;
			const u32 want = (before[1] & ~(0xFFu << sh)) | (v << sh);
			if (words[0] != before[0] || words[2] != before[2] || words[1] != want) {
				mismatch("byte_sat_inc", b, (u64)i, 0, words[1]);
			}
		}
		if (v != 255) {
			mismatch("byte_sat_inc: not at 255", b, 0, 0, v);
		}
	}
}

int
selftest()
{
	Lds s;
	s.codes = static_cast<u8*>(std::malloc(TILE_LDS_BYTES));
	if (!s.codes) {
		return 2;
	}
	const u32 ks[] = { 12, 13, 14, 15, 25, 64, 65, 199, 200, 255, 256 };
	for (u32 k : ks) {
		u64 tabs[TAB_WORDS];
		build_seed_tables(k, tabs);
		const unsigned long long starts0 = g_starts, valid0 = g_valid, mis0 = g_mismatches;
		const u64 T = TILE_STARTS;
		const u64 ns[] = { 0, 1, k - 1, k, T, T + k - 1, T + k, 2 * T + 5 };
		for (u64 n : ns) {
			check_batch(s, tabs, k, n, 0);
		}
		for (int variant = 1; variant < 4; variant++) { // every odd byte at every place, on the batch that has them all
			check_batch(s, tabs, k, 2 * T + 5, variant);
		}
		check_entries(k);
		std::printf("k %u: starts %llu valid %llu mismatches %llu\n", k, g_starts - starts0, g_valid - valid0, g_mismatches - mis0);
	}
	check_bit_range();
	check_byte_sat_inc();
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
	std::fprintf(stderr, "usage: tile_host selftest\n");
	return 2;
}
