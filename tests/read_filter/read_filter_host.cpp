// read_filter_host.cpp -- --min_read_len, --min_mean_qual and --min_rq on the host, as a program of its own: the two
// serial models (rp_model_f of nte_reads_model.h, bam_model_f of nte_bam_grammar.h) and the filtering FastaReader
// (ntedit_amd/host/fasta.cpp), built by tests/test_read_filter_cpu.py with and without -fsanitize=address,undefined.
// No HIP, no library.
//
//   read_filter_host CASES SCRATCH
// CASES: per case u32 kind, u32 k (the BAM model: min_len), u32 min_qual, u32 min_read_len, u32 min_mean_qual, f32 min_rq,
// u64 n, then n bytes.  Every input is copied into a heap block of its exact size, so a read past a quality string or an
// aux field cut short is reported.  One line per case:
//   kind 0 (the text parser's model)   clean broken text_len reads fold records by_length by_mean_qual
//   kind 1 (the BAM model, at_header)  clean broken cut kept text_len fold records by_length by_rq by_mean_qual rq_tagged
//                                      aux_malformed
//   kind 2 (FastaReader over SCRATCH, which the bytes are written to; min_len = max(min_read_len, k))
//                                      reads text_len fold records by_length by_mean_qual failed
// fold: the text's bytes folded as f = f * 31 + b (mod 2^32).
#include "nte_bam_grammar.h"
#include "nte_reads_model.h"

#include "../../ntedit_amd/host/fasta.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

typedef unsigned long long ull;

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
		fprintf(stderr, "usage: read_filter_host CASES SCRATCH\n");
		return 2;
	}
	FILE* fp = fopen(argv[1], "rb");
	if (!fp) {
		return 2;
	}
	for (;;) {
		uint32_t head[6];
		uint64_t n = 0;
		if (fread(head, 4, 6, fp) != 6 || fread(&n, 8, 1, fp) != 1) {
			break;
		}
		char* raw = (char*)malloc(n ? n : 1);
		if (n && fread(raw, 1, n, fp) != n) {
			return 2;
		}
		const uint32_t kind = head[0], k = head[1], q = head[2];
		nte_parse::ReadFilter f = nte_parse::ReadFilter();
		f.min_len = head[3];
		f.min_mean_qual = head[4];
		f.rq_bits = head[5];
		nte_parse::ReadFilterCounts fc = nte_parse::ReadFilterCounts();
		if (kind == 0) {
			const uint64_t cap = n + 1;
			char* out = (char*)malloc(cap);
			nte_parse::RpResult r;
			if (!nte_parse::rp_model_f(raw, n, k, q, f, out, cap, &r, &fc)) {
				return 3;
			}
			printf("%d %u %llu %llu %u %llu %llu %llu\n", r.clean, r.broken, (ull)r.text_len, (ull)r.reads, fold(0, out, r.text_len),
			       (ull)fc.records, (ull)fc.by_length, (ull)fc.by_mean_qual);
			free(out);
		} else if (kind == 1) {
			const uint64_t cap = n + 1;
			char* out = (char*)malloc(cap);
			nte_bam::BamResult r;
			nte_bam::bam_model_f((const uint8_t*)raw, n, 1, k, q, f, out, cap, &r, nullptr, &fc);
			printf("%d %u %llu %llu %llu %u %llu %llu %llu %llu %llu %llu\n", r.clean, r.broken, (ull)r.cut, (ull)r.kept, (ull)r.text_len,
			       fold(0, out, r.clean ? r.text_len : 0), (ull)fc.records, (ull)fc.by_length, (ull)fc.by_rq, (ull)fc.by_mean_qual,
			       (ull)fc.rq_tagged, (ull)fc.aux_malformed);
			free(out);
		} else {
			FILE* w = fopen(argv[2], "wb");
			if (!w || (n && fwrite(raw, 1, n, w) != n) || fclose(w) != 0) {
				return 2;
			}
			nte_host::FastaReader reader(argv[2]);
			reader.set_min_qual(q);
			nte_parse::ReadFilter host = f;
			host.min_len = nte_parse::rp_min_len(f, k);
			host.rq_bits = 0;
			reader.set_read_filter(host);
			std::string hdr, seq;
			uint64_t reads = 0, text = 0;
			uint32_t fo = 0;
			for (;;) {
				seq.clear();
				if (!reader.next(hdr, seq)) {
					break;
				}
				const unsigned why = reader.drop_reason();
				fc.records++;
				fc.by_length += why == nte_parse::RP_DROP_LENGTH;
				fc.by_mean_qual += why == nte_parse::RP_DROP_MEAN_QUAL;
				if (why != nte_parse::RP_KEPT) {
					continue;
				}
				seq.push_back('\n');
				fo = fold(fo, seq.data(), seq.size());
				reads++;
				text += seq.size();
			}
			printf("%llu %llu %u %llu %llu %llu %d\n", (ull)reads, (ull)text, fo, (ull)fc.records, (ull)fc.by_length, (ull)fc.by_mean_qual,
			       reader.next_start() == ~0ull ? 1 : 0);
		}
		free(raw);
	}
	fclose(fp);
	return 0;
}
