// model_host.cpp -- nte_bam_grammar.h alone, as a host program (no HIP, no library): the serial model and the check behind
// ntedit_hip_reads_is_bam over a file of cases, one result line per case.  tests/test_reads_bam_cpu.py builds it with
// -fsanitize=address,undefined and compares the lines with the Python restatement.  Every input and output is a heap
// block of its exact size, so a read or write past an end is reported.
//
// cases file: per case  u32 kind (0: the model, 1: the start of a file), u32 at_header, u32 min_len, u64 n, n bytes
#include "nte_bam_grammar.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int
main(int argc, char** argv)
{
	if (argc != 2) {
		fprintf(stderr, "usage: model_host cases.bin\n");
		return 2;
	}
	FILE* fp = fopen(argv[1], "rb");
	if (!fp) {
		fprintf(stderr, "cannot open %s\n", argv[1]);
		return 2;
	}
	unsigned long long cases = 0;
	for (;;) {
		uint32_t head[3];
		uint64_t n = 0;
		if (fread(head, 4, 3, fp) != 3) {
			break;
		}
		if (fread(&n, 8, 1, fp) != 1) {
			return 2;
		}
		uint8_t* raw = (uint8_t*)malloc(n ? n : 1);
		if (n && fread(raw, 1, n, fp) != n) {
			return 2;
		}
		if (head[0] == 1) {
			printf("%d\n", nte_bam::bam_starts_bam(raw, n) ? 1 : 0);
		} else {
			const uint64_t cap = n + 1;
			char* out = (char*)malloc(cap);
			nte_bam::BamResult r;
			nte_bam::bam_model(raw, n, (int)head[1], head[2], out, cap, &r);
			uint32_t sum = 0; // (the text, folded: the test has it from the library's model)
			for (uint64_t i = 0; r.clean && i < r.text_len && i < cap; i++) {
				sum = sum * 31 + (uint8_t)out[i];
			}
			printf("%d %u %llu %u %llu %llu %llu %llu %llu %llu %llu %u\n", r.clean, r.broken, (unsigned long long)r.header_len, r.n_ref,
			       (unsigned long long)r.cut, (unsigned long long)r.records, (unsigned long long)r.kept, (unsigned long long)r.skipped_flag,
			       (unsigned long long)r.skipped_short, (unsigned long long)r.bases, (unsigned long long)r.text_len, sum);
			free(out);
		}
		free(raw);
		cases++;
	}
	fclose(fp);
	fprintf(stderr, "cases %llu\n", cases);
	return 0;
}
