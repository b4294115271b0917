// settle_host.cpp -- TEST-ONLY: settle_event() (ntedit_amd/csrc/nte_settle.h) against the event machine, on the CPU.
//
// Every event of a batch goes through MachineT::run + finish and through settle_event().  Wherever settle_event()
// accepts, the machine's arena chunk (four items), its cover end and its flags must equal what settle_event() returned,
// byte for byte; where it declines, its output must be untouched.
//
//   settle_host selftest            planted cases over a grid of parameters, seeded random cases, the i.i.d. case
//   settle_host count BLOB BF K H [JUMP [GRID]]   a batch ('\n' behind every contig) and the raw bits of a plain filter from files
// Both print "events E settled S mismatches M"; the exit status is 1 when M > 0.
#include "../../ntedit_amd/csrc/nte_machine.h"
#include "../../ntedit_amd/csrc/nte_settle.h"
#include "../../ntedit_amd/host/params.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace nte;

namespace {

struct Rng
{
	u64 s;
	explicit Rng(u64 seed)
	  : s(seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL)
	{
	}
	u64 next()
	{
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return s;
	}
	u32 below(u32 n) { return (u32)((next() >> 11) % n); }
	double unit() { return (double)(next() >> 11) / 9007199254740992.0; }
};

const char ACGT[] = "ACGT";

std::string
random_seq(Rng& r, size_t n)
{
	std::string s(n, 'A');
	for (size_t i = 0; i < n; i++) {
		s[i] = ACGT[r.below(4)];
	}
	return s;
}

char
other_base(Rng& r, char c)
{
	char o;
	do {
		o = ACGT[r.below(4)];
	} while (o == c);
	return o;
}

std::string
mutate(Rng& r, const std::string& t, double p_sub, double p_indel)
{
	std::string d;
	for (size_t i = 0; i < t.size();) {
		const double x = r.unit();
		if (x < p_sub) {
			d += other_base(r, t[i]);
			i++;
		} else if (x < p_sub + p_indel / 2) {
			const u32 l = 1 + r.below(3);
			for (u32 q = 0; q < l; q++) {
				d += ACGT[r.below(4)];
			}
		} else if (x < p_sub + p_indel) {
			i += 1 + r.below(3);
		} else {
			d += t[i];
			i++;
		}
	}
	return d;
}

struct Setup
{
	DevParams p;
	u64 tab[TAB_WORDS];
	std::vector<u8> bits;
	Filter f;

	bool init(u32 k, u32 h, u32 jump, u32 grid, u64 bf_bytes)
	{
		ntedit_hip_params hp;
		nte_host::params_default(&hp);
		hp.jump = jump;
		hp.start_grid = grid;
		if (nte_host::make_dev_params(hp, k, h, false, &p, false)) {
			return false;
		}
		build_seed_tables(k, tab);
		bits.assign(bf_bytes, 0);
		bind();
		return true;
	}
	void bind()
	{
		f.data = bits.data();
		filter_set_size(f, (u64)bits.size() * 8);
		f.hash_num = p.h;
		f.counting = 0;
	}
	void clear() { std::fill(bits.begin(), bits.end(), 0); }
	// every k-mer of accepted bases of s
	void insert(const std::string& s)
	{
		HashState hs = { 0, 0 };
		u64 good = 0;
		for (size_t i = 0; i < s.size(); i++) {
			const u8 in = char_code((u8)s[i]);
			const u8 out = i >= p.k ? char_code((u8)s[i - p.k]) : CODE_BAD;
			hash_roll(hs, tab, out, in);
			good = in == CODE_BAD ? 0 : good + 1;
			if (good >= p.k) {
				for (u32 q = 0; q < p.h; q++) {
					const u64 n = filter_slot(f, hash_extend(hs.fh + hs.rh, p, q));
					bits[n >> 3] |= (u8)(1u << (n & 7));
				}
			}
		}
	}
};

struct Tally
{
	u64 events = 0, settled = 0, mismatches = 0;
	void add(const Tally& o)
	{
		events += o.events;
		settled += o.settled;
		mismatches += o.mismatches;
	}
};

void
sim_screen(const u8* seq, u64 n, const Filter& f, const DevParams& p, const u64* tab, u64* bitmap)
{
	HashState hs = { 0, 0 };
	u64 good = 0;
	for (u64 i = 0; i < n; i++) {
		const u8 in = char_code(seq[i]);
		const u8 out = i >= p.k ? char_code(seq[i - p.k]) : CODE_BAD;
		hash_roll(hs, tab, out, in);
		good = in == CODE_BAD ? 0 : good + 1;
		if (good >= p.k && filter_screen_absent(f, p, hs)) {
			const u64 s = i + 1 - p.k;
			bitmap[s >> 6] |= 1ULL << (s & 63);
		}
	}
}

template<u32 CFG>
bool
same_as_machine(EventEnv env, u32 start, bool accepted, const SettleOut& out, const char* what)
{
	if (!accepted) {
		return true;
	}
	u32 arena_next = 0;
	env.arena_next = &arena_next;
	MachineT<CFG> m(env);
	u32 cover_end = start;
	m.template run<false>(start, cover_end);
	const u32 fc = m.finish(start, cover_end);
	const bool ok = m.flags == 0 && fc == 0 && arena_next == 1 && cover_end == out.cover_end &&
	                memcmp(env.arena, out.item, sizeof out.item) == 0;
	if (!ok) {
		fprintf(stderr, "MISMATCH (%s, machine cfg %u): k %u jump %u h %u contig %u start %u: machine flags %u first chunk %u chunks %u cover %u, settled cover %u\n",
		        what, CFG, env.p->k, env.p->jump, env.p->h, env.contig, start, m.flags, fc, arena_next, cover_end, out.cover_end);
	}
	return ok;
}

// every event of the batch (contigs, each followed by '\n') through the machine and through settle_event()
Tally
run_batch(const Setup& su, const std::vector<std::string>& contigs, const char* what)
{
	Tally t;
	const DevParams& p = su.p;
	// (the batch buffer starts 8-byte aligned: the window is read in aligned words)
	std::vector<u64> store;
	std::vector<u64> offsets;
	std::vector<u32> lens;
	u64 n = 0;
	for (const std::string& c : contigs) {
		offsets.push_back(n);
		lens.push_back((u32)c.size());
		n += c.size() + 1;
	}
	store.assign(n / 8 + 2, 0);
	u8* blob = (u8*)store.data();
	for (size_t i = 0; i < contigs.size(); i++) {
		memcpy(blob + offsets[i], contigs[i].data(), contigs[i].size());
		blob[offsets[i] + contigs[i].size()] = '\n';
	}
	std::vector<u64> bitmap((n + 63) / 64 + 9, 0);
	sim_screen(blob, n, su.f, p, su.tab, bitmap.data());

	std::vector<Node> nodes(p.node_window);
	std::vector<u32> ov_pos(p.node_window);
	std::vector<u8> ov_chr(p.node_window);
	std::vector<u8> win(2 * p.k + p.max_deletions + 8 + 32 + 64);
	std::vector<u8> swin(2 * p.k);
	std::vector<u8> prev(p.node_window);
	std::vector<int16_t> lps(p.node_window);
	const u32 arena_chunks = 4096;
	std::vector<Item> arena((size_t)arena_chunks * CHUNK_ITEMS);

	size_t ci = 0;
	for (u64 g = 0; g < n; g++) {
		if (!is_event_start(bitmap.data(), g, p.start_grid)) {
			continue;
		}
		while (ci + 1 < contigs.size() && offsets[ci + 1] <= g) {
			ci++;
		}
		EventEnv env;
		memset(&env, 0, sizeof env);
		env.seq = blob + offsets[ci];
		env.batch_end = blob + n;
		env.len = lens[ci];
		env.contig = (u32)ci;
		env.gbase = offsets[ci];
		env.bitmap = bitmap.data();
		env.runmap = bitmap.data();
		env.tab = su.tab;
		env.p = &p;
		env.bloom = su.f;
		env.rep = su.f;
		env.nodes = nodes.data();
		env.ov_pos = ov_pos.data();
		env.ov_chr = ov_chr.data();
		env.win = win.data();
		env.win_stride = 1;
		env.prev = prev.data();
		env.lps = lps.data();
		env.arena = arena.data();
		env.arena_chunks = arena_chunks;
		env.defer_sweeps = false;
		env.wave_size = 1;
		const u32 start = (u32)(g - offsets[ci]);
		if ((u64)start + p.k > env.len) {
			continue; // (k_machine does not run these)
		}
		t.events++;

		SettleOut out, untouched;
		memset(&out, 0xA5, sizeof out);
		memset(&untouched, 0xA5, sizeof untouched);
		EventEnv senv = env;
		senv.win = swin.data();
		bool acc = settle_applicable(p, su.f) && settle_event<8>(senv, start, out);
		// (the group size is a matter of speed only)
		SettleOut out13;
		memset(&out13, 0xA5, sizeof out13);
		const bool acc13 = settle_applicable(p, su.f) && settle_event<13>(senv, start, out13);
		bool ok = acc == acc13 && memcmp(&out, &out13, sizeof out) == 0;
		if (!acc && memcmp(&out, &untouched, sizeof out) != 0) {
			fprintf(stderr, "MISMATCH (%s): a declined event wrote its output, contig %zu start %u\n", what, ci, start);
			ok = false;
		}
		ok = same_as_machine<0>(env, start, acc, out, what) && ok;
		if (su.f.mask) {
			ok = same_as_machine<15>(env, start, acc, out, what) && ok; // the instantiation a power-of-two filter runs on
		}
		t.settled += acc ? 1 : 0;
		t.mismatches += ok ? 0 : 1;
	}
	return t;
}

// ---- planted cases for one parameter set
Tally
planted(Setup& su, u64 seed)
{
	Tally t;
	Rng r(seed);
	const u32 k = su.p.k;
	const u32 md = su.p.max_deletions;
	const std::string truth = random_seq(r, 40 * k + 4000);
	auto piece = [&](u32 len) {
		const u32 at = r.below((u32)truth.size() - len);
		return truth.substr(at, len);
	};
	auto sub_at = [&](std::string& d, size_t q) { d[q] = other_base(r, d[q]); };

	// two substitutions at every distance 1 .. 2k + 2
	{
		su.clear();
		su.insert(truth);
		std::vector<std::string> cs;
		for (u32 d = 1; d <= 2 * k + 2; d++) {
			std::string c = piece(8 * k);
			sub_at(c, 3 * k);
			sub_at(c, 3 * k + d);
			cs.push_back(c);
		}
		t.add(run_batch(su, cs, "two substitutions"));
	}
	// one substitution at every distance from a contig's end and start, contigs of 2k .. 4k bases
	{
		std::vector<std::string> cs;
		for (u32 d = 0; d <= 2 * k + md + 10; d++) {
			for (u32 L = 2 * k; L <= 4 * k; L += k / 2) {
				if (d >= L) {
					continue;
				}
				std::string a = piece(L), b = piece(L);
				sub_at(a, L - 1 - d);
				sub_at(b, d);
				cs.push_back(a);
				cs.push_back(b);
			}
		}
		t.add(run_batch(su, cs, "contig ends"));
	}
	// a lower-case error base; N and IUPAC codes at every window offset (the window starts k - 1 in front of the error)
	{
		std::vector<std::string> cs;
		std::string c = piece(8 * k);
		sub_at(c, 4 * k);
		c[4 * k] = (char)(c[4 * k] + 32);
		cs.push_back(c);
		c = piece(8 * k);
		for (u32 q = 3 * k; q < 5 * k; q++) {
			c[q] = (char)(c[q] + 32); // (lower-case all around, the error base upper-case)
		}
		sub_at(c, 4 * k);
		c[4 * k] = (char)(c[4 * k] & 0xDF);
		cs.push_back(c);
		const char odd[] = "NRYSWKMBDHVn";
		for (u32 o = 0; o <= 2 * k + 3; o++) {
			for (int v = 0; v < 2; v++) {
				c = piece(8 * k);
				const u32 s = 4 * k;
				sub_at(c, s);
				const u32 q = s - (k - 1) + o;
				if (q == s) {
					c[q] = v ? 'N' : odd[1 + r.below(10)]; // the error position itself reads N / an IUPAC code
				} else {
					c[q] = v ? odd[r.below(12)] : 'N';
				}
				cs.push_back(c);
			}
		}
		t.add(run_batch(su, cs, "characters"));
	}
	// decoy candidates: the draft k-mer with another last base is in the filter
	for (int variant = 0; variant < 2; variant++) { // 0: its own k-mer only, 1: fully supported
		// every draft base, every true base, each of the two bases left as the decoy: in candidate order the decoy
		// stands in front of the true base in 12 of the 24 cases and behind it in the other 12 (counted below)
		u32 in_front = 0, behind = 0;
		for (int di = 0; di < 4; di++) {
			for (int gi = 0; gi < 4; gi++) {
				if (gi == di) {
					continue;
				}
				const char draft = ACGT[di], good = ACGT[gi];
				su.clear();
				su.insert(truth);
				const u32 s = 4 * k;
				std::string c = piece(8 * k);
				while (c[s] != good) {
					c = piece(8 * k);
				}
				c[s] = draft;
				u8 cand[MAX_CANDIDATES];
				const u32 n_cand = SettleMachine::candidate_bases((u8)draft, false, cand);
				std::vector<std::string> cs;
				for (int w = 0; w < 4; w++) {
					const char decoy = ACGT[w];
					if (decoy == good || decoy == draft) {
						continue;
					}
					u32 at_decoy = n_cand, at_good = n_cand;
					for (u32 q = 0; q < n_cand; q++) {
						at_decoy = cand[q] == (u8)decoy ? q : at_decoy;
						at_good = cand[q] == (u8)good ? q : at_good;
					}
					if (at_decoy == n_cand || at_good == n_cand) {
						fprintf(stderr, "MISMATCH (decoy): %c or %c is no candidate of %c\n", decoy, good, draft);
						t.mismatches++;
					}
					(at_decoy < at_good ? in_front : behind)++;
					Setup one = su;
					one.bind();
					std::string dk = c.substr(s - (k - 1), variant ? 2 * k - 1 : k);
					dk[k - 1] = decoy;
					one.insert(dk);
					cs.assign(1, c);
					t.add(run_batch(one, cs, variant ? "decoy with full support" : "decoy of one k-mer"));
				}
			}
		}
		if (in_front != 12 || behind != 12) {
			fprintf(stderr, "MISMATCH (decoy): %u decoys in front of the true base, %u behind it\n", in_front, behind);
			t.mismatches++;
		}
	}
	// exactly one k-mer start + i of the corrected sequence is missing, i = 1 .. k: the filter from two truth pieces
	for (u32 i = 1; i <= k; i++) {
		std::string tr = piece(8 * k);
		std::string c = tr;
		const u32 s = 4 * k, start = s - (k - 1);
		sub_at(c, s);
		su.clear();
		su.insert(tr.substr(0, start + i + k - 1));
		su.insert(tr.substr(start + i + 1));
		std::vector<std::string> cs(1, c);
		t.add(run_batch(su, cs, "one missing k-mer"));
	}
	return t;
}

Tally
random_case(Setup& su, u64 seed, size_t n, double p_sub, double p_indel, bool odd_chars)
{
	Rng r(seed);
	const std::string truth = random_seq(r, n);
	su.clear();
	su.insert(truth);
	std::vector<std::string> cs;
	for (int part = 0; part < 3; part++) {
		std::string d = mutate(r, truth.substr(part * (n / 3), n / 3), p_sub, p_indel);
		if (odd_chars) {
			for (int q = 0; q < 40; q++) {
				d[r.below((u32)d.size())] = "NRYSWKMBDHVacgtn"[r.below(16)];
			}
		}
		cs.push_back(d);
	}
	return run_batch(su, cs, "random");
}

std::vector<u8>
read_file(const char* path)
{
	std::vector<u8> v;
	FILE* f = fopen(path, "rb");
	if (!f) {
		return v;
	}
	u8 buf[1 << 16];
	size_t got;
	while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
		v.insert(v.end(), buf, buf + got);
	}
	fclose(f);
	return v;
}

} // namespace

int
main(int argc, char** argv)
{
	Tally all;
	if (argc >= 6 && !strcmp(argv[1], "count")) {
		const std::vector<u8> blob = read_file(argv[2]);
		Setup su;
		if (!su.init((u32)atoi(argv[4]), (u32)atoi(argv[5]), argc > 6 ? (u32)atoi(argv[6]) : 3, argc > 7 ? (u32)atoi(argv[7]) : 0, 8)) {
			fprintf(stderr, "bad parameters\n");
			return 2;
		}
		su.bits = read_file(argv[3]);
		su.bind();
		std::vector<std::string> cs;
		size_t a = 0;
		for (size_t i = 0; i < blob.size(); i++) {
			if (blob[i] == '\n') {
				cs.emplace_back((const char*)blob.data() + a, i - a);
				a = i + 1;
			}
		}
		all = run_batch(su, cs, "file");
	} else if (argc >= 2 && !strcmp(argv[1], "selftest")) {
		const u32 ks[] = { 12, 25, 32, 33, 64 }, jumps[] = { 1, 3 }, hs[] = { 1, 3, 4 }, grids[] = { 0, 4 };
		u64 seed = 1;
		for (u32 k : ks) {
			for (u32 jump : jumps) {
				for (u32 h : hs) {
					for (u32 grid : grids) {
						Setup su;
						// (a size that is no power of two; a power of two with the default grid at -j 3: the specialised machine)
						const u64 bytes = (grid == 0 && jump == 3) ? (1u << 17) : 100003;
						if (!su.init(k, h, jump, grid, bytes)) {
							fprintf(stderr, "bad parameters\n");
							return 2;
						}
						Tally t = planted(su, seed++);
						t.add(random_case(su, seed, 60000, 5e-3, 1e-3, h != 3));
						seed++;
						printf("k %u jump %u h %u grid %u filter %llu bytes: events %llu settled %llu mismatches %llu\n", k, jump, h, su.p.start_grid,
						       (unsigned long long)bytes, (unsigned long long)t.events, (unsigned long long)t.settled, (unsigned long long)t.mismatches);
						all.add(t);
					}
				}
			}
		}
		// the i.i.d. case: 2 Mbp, 0.5 % substitutions, 0.05 % indels, k = 25, h = 3, a 16 MiB filter
		Setup su;
		if (!su.init(25, 3, 3, 0, 16u << 20)) {
			return 2;
		}
		const Tally t = random_case(su, 4242, 2000000, 5e-3, 5e-4, false);
		printf("iid: events %llu settled %llu mismatches %llu share %.4f\n", (unsigned long long)t.events, (unsigned long long)t.settled,
		       (unsigned long long)t.mismatches, t.events ? (double)t.settled / (double)t.events : 0.0);
		all.add(t);
	} else {
		fprintf(stderr, "usage: settle_host selftest | count BLOB BF K H [JUMP [GRID]]\n");
		return 2;
	}
	printf("events %llu settled %llu mismatches %llu\n", (unsigned long long)all.events, (unsigned long long)all.settled, (unsigned long long)all.mismatches);
	return all.mismatches ? 1 : 0;
}
