// unit_host.cpp -- the HIP-free parts of ntedit_amd/csrc/nte_reads_unit.h (the per-context registry, the Keep / Scratch
// state, the carver) and the two host helpers of nte_reads_grammar.h (rp_make_filter, rp_counts_add) on the CPU, alone.
// tests/test_reads_unit_cpu.py builds this program plain, with -fsanitize=address,undefined and with -fsanitize=thread,
// and runs each check by name; a check prints "ok" or what failed and where.  Nothing of the library is linked.
//
//   registry   one state per owner, the same state on the next lookup, null without `create` for an unknown owner
//   threads    eight threads create states for the same 16 owners at once: 16 states, every thread got the same ones
//   scratch    `scr = Scratch()` leaves Keep as it was
//   filter     rp_make_filter against the three inline tests it replaced, restated below, over the edge arguments
//   counts     rp_counts_add adds all six fields
//   carver     parts at multiples of 256, none overlapping, the total the sum of the rounded sizes; a null base only sizes
#include "../../ntedit_amd/csrc/nte_reads_grammar.h"
#include "../../ntedit_amd/csrc/nte_reads_unit.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <thread>

using namespace nte_parse;
using namespace nte_unit;

namespace {

int g_failed = 0;

#define CHECK(cond)                                                 \
	do {                                                            \
		if (!(cond)) {                                              \
			printf("FAILED line %d: %s\n", __LINE__, #cond);        \
			g_failed++;                                             \
		}                                                           \
	} while (0)

struct Keep
{
	int on = 0;
	uint64_t count = 0;
};

struct Scratch
{
	int device = -1;
	void* p = nullptr;
	uint64_t cap = 0;
};

typedef State<Keep, Scratch> S;

void
check_registry()
{
	Registry<S> reg;
	int owners[3];
	CHECK(reg.size() == 0);
	CHECK(reg.find(&owners[0], false) == nullptr);
	CHECK(reg.size() == 0); // (a lookup without `create` makes nothing)
	S* a = reg.find(&owners[0], true);
	S* b = reg.find(&owners[1], true);
	CHECK(a && b && a != b);
	CHECK(a->owner == &owners[0] && b->owner == &owners[1]);
	CHECK(reg.find(&owners[0], true) == a && reg.find(&owners[0], false) == a);
	CHECK(reg.find(&owners[1], false) == b);
	CHECK(reg.find(&owners[2], false) == nullptr);
	CHECK(reg.size() == 2);
	// a new state is default-constructed on both sides
	CHECK(a->keep.on == 0 && a->keep.count == 0 && a->scr.device == -1 && a->scr.p == nullptr && a->scr.cap == 0);
	// the states are apart: what one context sets the other does not see
	a->keep.on = 1;
	CHECK(b->keep.on == 0);
}

void
check_threads()
{
	static Registry<S> reg;
	constexpr int THREADS = 8, OWNERS = 16;
	static int owners[OWNERS];
	static S* got[THREADS][OWNERS];
	std::thread th[THREADS];
	for (int t = 0; t < THREADS; t++) {
		th[t] = std::thread([t] {
			for (int i = 0; i < OWNERS; i++) {
				const int o = (i + t) % OWNERS; // (each thread starts at another owner)
				got[t][o] = reg.find(&owners[o], true);
			}
		});
	}
	for (std::thread& x : th) {
		x.join();
	}
	CHECK(reg.size() == OWNERS);
	for (int o = 0; o < OWNERS; o++) {
		CHECK(got[0][o] && got[0][o]->owner == &owners[o]);
		for (int t = 1; t < THREADS; t++) {
			CHECK(got[t][o] == got[0][o]);
		}
		for (int p = 0; p < o; p++) {
			CHECK(got[0][p] != got[0][o]);
		}
	}
}

void
check_scratch()
{
	S s;
	int owner;
	s.owner = &owner;
	s.keep.on = 1;
	s.keep.count = 1234567890123ull;
	s.scr.device = 3;
	s.scr.p = &owner;
	s.scr.cap = 99;
	s.scr = Scratch();
	CHECK(s.owner == &owner && s.keep.on == 1 && s.keep.count == 1234567890123ull);
	CHECK(s.scr.device == -1 && s.scr.p == nullptr && s.scr.cap == 0);
}

// the three tests rp_make_filter replaced, as they stood in ntedit_hip_reads_set_read_filter, ntedit_hip_reads_parse_model_f
// and ntedit_hip_reads_bam_model_f (the same text three times; the BAM one with the namespace spelled out)
bool
old_set_read_filter_refuses(uint32_t min_len, uint32_t min_mean_qual, float min_rq)
{
	return min_len > RP_MAX_MIN_READ_LEN || min_mean_qual > RP_MAX_MEAN_QUAL || !(min_rq >= 0.0f && min_rq <= 1.0f);
}

bool
old_parse_model_refuses(uint32_t min_len, uint32_t min_mean_qual, float min_rq)
{
	return min_len > RP_MAX_MIN_READ_LEN ||
	       min_mean_qual > RP_MAX_MEAN_QUAL || !(min_rq >= 0.0f && min_rq <= 1.0f);
}

bool
old_bam_model_refuses(uint32_t min_read_len, uint32_t min_mean_qual, float min_rq)
{
	return min_read_len > nte_parse::RP_MAX_MIN_READ_LEN ||
	       min_mean_qual > nte_parse::RP_MAX_MEAN_QUAL || !(min_rq >= 0.0f && min_rq <= 1.0f);
}

void
check_filter()
{
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const uint32_t lens[] = { 0, 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu };
	const uint32_t quals[] = { 0, 1, 60, 61, 0xFFFFFFFFu };
	const float rqs[] = { 0.0f, -0.0f, 1.0f, std::nextafter(1.0f, 2.0f), 1.5f, -0.25f, std::nextafter(0.0f, 1.0f), 0.9f, nan, -nan, inf, -inf };
	static_assert(RP_MAX_MIN_READ_LEN == 0x7FFFFFFFu && RP_MAX_MEAN_QUAL == 60, "the maxima the lists above are written around");
	int accepted = 0, refused = 0;
	for (uint32_t len : lens) {
		for (uint32_t q : quals) {
			for (float rq : rqs) {
				ReadFilter f = { 7, 7, 7 };
				const bool ok = rp_make_filter(len, q, rq, &f);
				const bool old = old_set_read_filter_refuses(len, q, rq);
				CHECK(old == old_parse_model_refuses(len, q, rq) && old == old_bam_model_refuses(len, q, rq));
				CHECK(ok == !old);
				if (ok) {
					// ... and what the callers then built by hand
					CHECK(f.min_len == len && f.min_mean_qual == q && f.rq_bits == rp_rq_bits(rq));
					accepted++;
				} else {
					CHECK(f.min_len == 7 && f.min_mean_qual == 7 && f.rq_bits == 7); // (a refused argument writes nothing)
					refused++;
				}
			}
		}
	}
	CHECK(accepted == 3 * 3 * 5 && refused == 5 * 5 * 12 - accepted); // (0, 1, max of each; rq 0, -0, 1, the smallest positive, 0.9)
	ReadFilter f = {};
	CHECK(rp_make_filter(40, 15, 0.9f, &f) && f.min_len == 40 && f.min_mean_qual == 15);
	float back;
	memcpy(&back, &f.rq_bits, 4);
	CHECK(back == 0.9f);
	CHECK(rp_make_filter(0, 0, -0.0f, &f) && f.rq_bits == 0 && !rp_filter_on(f)); // (-0.0 is off, not a filter of its bits)
}

void
check_counts()
{
	ReadFilterCounts to = { 1, 2, 3, 4, 5, 6 };
	const ReadFilterCounts add = { 10, 200, 3000, 40000, 500000, 1ull << 40 };
	rp_counts_add(&to, add);
	CHECK(to.records == 11 && to.by_length == 202 && to.by_rq == 3003 && to.by_mean_qual == 40004 && to.rq_tagged == 500005 &&
	      to.aux_malformed == (1ull << 40) + 6);
	rp_counts_add(&to, ReadFilterCounts()); // (what the text parser adds for the three fields it leaves at zero)
	CHECK(to.records == 11 && to.by_rq == 3003 && to.rq_tagged == 500005 && to.aux_malformed == (1ull << 40) + 6);
	CHECK(add.records == 10 && add.aux_malformed == 1ull << 40);
}

void
check_carver()
{
	CHECK(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);
	CHECK(up256((1ull << 40) + 1) == (1ull << 40) + 256);
	const uint64_t sizes[] = { 1, 255, 256, 257, 0, 4096, 3, 1000 };
	constexpr int N = sizeof sizes / sizeof sizes[0];
	Carver sizing(nullptr);
	uint64_t sum = 0;
	for (uint64_t n : sizes) {
		CHECK(sizing.take(n) == nullptr);
		sum += up256(n);
	}
	CHECK(sizing.at == sum);
	// the same parts of a real allocation (exactly as large: a sanitizer sees a byte past a part's rounded size)
	uint8_t* base = new uint8_t[sum];
	Carver cut(base);
	uint8_t* part[N];
	for (int i = 0; i < N; i++) {
		part[i] = cut.take(sizes[i]);
		CHECK((uint64_t)(part[i] - base) % 256 == 0);
		CHECK(i == 0 ? part[i] == base : part[i] == part[i - 1] + up256(sizes[i - 1])); // (behind its predecessor: no overlap, no gap but the rounding)
		CHECK((uint64_t)(part[i] - base) + sizes[i] <= sum);
		memset(part[i], i + 1, sizes[i]);
	}
	CHECK(cut.at == sum && cut.at == sizing.at);
	for (int i = 0; i < N; i++) { // no later part wrote into an earlier one
		for (uint64_t b = 0; b < sizes[i]; b++) {
			if (part[i][b] != i + 1) {
				CHECK(part[i][b] == i + 1);
				break;
			}
		}
	}
	delete[] base;
}

} // namespace

int
main(int argc, char** argv)
{
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "registry") {
		check_registry();
	} else if (what == "threads") {
		check_threads();
	} else if (what == "scratch") {
		check_scratch();
	} else if (what == "filter") {
		check_filter();
	} else if (what == "counts") {
		check_counts();
	} else if (what == "carver") {
		check_carver();
	} else {
		fprintf(stderr, "usage: unit_host registry|threads|scratch|filter|counts|carver\n");
		return 2;
	}
	if (g_failed == 0) {
		printf("ok\n");
	}
	return g_failed ? 1 : 0;
}
