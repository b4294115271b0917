// min_qual_host.cpp -- --min_qual on the host, as a program of its own: the two serial models (rp_model of
// nte_reads_model.h, bam_model_q of nte_bam_grammar.h) and the masking FastaReader (ntedit_amd/host/fasta.cpp), built by
// tests/test_min_qual_cpu.py with and without -fsanitize=address,undefined.  No HIP, no library.
//
//   min_qual_host CASES SCRATCH
// CASES: per case u32 kind, u32 k (the BAM model: min_len), u32 min_qual, u64 n, then n bytes.  Every input is copied
// into a heap block of its exact size, so a read past a quality string cut short is reported.  One line per case:
//   kind 0 (the text parser's model)   clean broken text_len reads bases fold
//   kind 1 (the BAM model, at_header)  clean broken cut kept text_len qual_bases masked_bases fold
//   kind 2 (FastaReader over SCRATCH, which the bytes are written to)
//                                      reads text_len qual_bases masked_bases failed fold
// fold: the text's bytes folded as f = f * 31 + b (mod 2^32); kind 2 keeps the records of k bases or more.
#include "nte_bam_grammar.h"
#include "nte_reads_model.h"

#include "../../ntedit_amd/host/fasta.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint32_t
fold(uint32_t f, const char* p, uint64_t n)
{
	for (uint64_t i = 0; i < n; i++) {
		f = f * 31u + (unsigned char)p[i];
	}
	return f;
}

int
main(int argc, char** argv)
{
	if (argc != 3) {
		fprintf(stderr, "usage: min_qual_host CASES SCRATCH\n");
		return 2;
	}
	FILE* fp = fopen(argv[1], "rb");
	if (!fp) {
		return 2;
	}
	for (;;) {
		uint32_t head[3];
		uint64_t n = 0;
		if (fread(head, 4, 3, fp) != 3 || fread(&n, 8, 1, fp) != 1) {
			break;
		}
		char* raw = (char*)malloc(n ? n : 1);
		if (n && fread(raw, 1, n, fp) != n) {
			return 2;
		}
		const uint32_t kind = head[0], k = head[1], q = head[2];
		if (kind == 0) {
			const uint64_t cap = n + 1;
			char* out = (char*)malloc(cap);
			nte_parse::RpResult r;
			if (!nte_parse::rp_model(raw, n, k, q, out, cap, &r)) {
				return 3;
			}
			printf("%d %u %llu %llu %llu %u\n", r.clean, r.broken, (unsigned long long)r.text_len, (unsigned long long)r.reads,
			       (unsigned long long)r.bases, fold(0, out, r.text_len));
			free(out);
		} else if (kind == 1) {
			const uint64_t cap = n + 1;
			char* out = (char*)malloc(cap);
			nte_bam::BamResult r;
			uint64_t counts[2] = { 0, 0 };
			nte_bam::bam_model_q((const uint8_t*)raw, n, 1, k, q, out, cap, &r, counts);
			printf("%d %u %llu %llu %llu %llu %llu %u\n", r.clean, r.broken, (unsigned long long)r.cut, (unsigned long long)r.kept,
			       (unsigned long long)r.text_len, (unsigned long long)counts[0], (unsigned long long)counts[1],
			       fold(0, out, r.clean ? r.text_len : 0));
			free(out);
		} else {
			FILE* w = fopen(argv[2], "wb");
			if (!w || (n && fwrite(raw, 1, n, w) != n) || fclose(w) != 0) {
				return 2;
			}
			nte_host::FastaReader reader(argv[2]);
			reader.set_min_qual(q);
			std::string hdr, seq;
			uint64_t reads = 0, text = 0, with_qual = 0, masked = 0;
			uint32_t f = 0;
			for (;;) {
				seq.clear();
				if (!reader.next(hdr, seq)) {
					break;
				}
				if (seq.size() < k) {
					continue;
				}
				seq.push_back('\n');
				f = fold(f, seq.data(), seq.size());
				reads++;
				text += seq.size();
				with_qual += reader.qual_bases();
				masked += reader.masked_bases();
			}
			printf("%llu %llu %llu %llu %d %u\n", (unsigned long long)reads, (unsigned long long)text, (unsigned long long)with_qual,
			       (unsigned long long)masked, reader.next_start() == ~0ull ? 1 : 0, f);
		}
		free(raw);
	}
	fclose(fp);
	return 0;
}
