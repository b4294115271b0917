// fasta.h -- streaming FASTA/FASTQ (optionally gzipped) reader for the host
// driver.  Record semantics follow what the reference gets from kseq
// (lib/kseq.h:176-215 as used at ntedit.cpp:2223-2230): name = header text up
// to the first whitespace, comment = the rest of the header line, sequence =
// all following lines concatenated.  Own implementation; the file is read (and inflated)
// block by block by a second thread, ahead of the parser.  A regular file that starts with
// the gzip magic is inflated by the decoder of gunzip.h (its member checksums verified by a
// third thread); everything else (plain text, pipes) goes through zlib's gzread.
#pragma once
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <zlib.h>

#include "../csrc/nte_reads_grammar.h" // (ReadFilter)

namespace nte_host {

class Gunzip;
// 1: inflate .gz inputs with zlib's gzread instead of the decoder of gunzip.h (A/B runs, tests); returns the old value
int set_gzip_through_zlib(int on);

class FastaReader
{
  public:
	explicit FastaReader(const char* path);
	// a byte range of a plain file: reading starts at byte `begin` (the caller puts it on a record start), and next()
	// stops before the first record whose first byte lies at or past `limit`
	FastaReader(const char* path, unsigned long long begin, unsigned long long limit);
	~FastaReader();
	bool ok() const { return f_ != nullptr || gz_ != nullptr; }
	// set once the input turned out to be unreadable half-way (corrupt or truncated .gz, I/O error): next()
	// then returns false as at the end of the file, and the caller must not treat what it got as the whole draft
	// (kseq, lib/kseq.h:103-107, treats a failed read as the end of the input; a polished genome that is silently shorter is worse)
	bool io_error() const { return io_error_; }
	const std::string& io_error_text() const { return io_error_text_; }
	// reads the next record; header = name [+ " " + comment]; the sequence is APPENDED to seq
	// (so a batch can be assembled without an intermediate copy); false at EOF
	bool next(std::string& header, std::string& seq);
	// once next() has returned false: the offset of the first byte of the record it stopped before (the limit's), the
	// offset of the end of the input if it ran out first, ~0 if a record failed to parse (plain files: file offsets)
	unsigned long long next_start() const { return next_start_; }
	// before the first next(): n bytes of the (inflated) input are read and dropped; offsets keep counting them
	void skip(unsigned long long n);
	// --min_qual (the reads passes alone; off by default, and a draft or a genome never sets it): next() masks the bases
	// of a FASTQ record by the quality string it walks anyway, the i-th quality character after concatenation against
	// the i-th base (nte_reads_grammar.h: rp_mask_base, Phred+33); a FASTA record passes as it is
	void set_min_qual(unsigned q) { min_qual_ = q; }
	// of the record the last next() returned: the bases that had a quality, and those of them below the minimum
	unsigned long long qual_bases() const { return qual_bases_; }
	unsigned long long masked_bases() const { return masked_bases_; }
	// --min_read_len, --min_mean_qual (the reads passes alone, like set_min_qual; min_len is the shortest record kept,
	// rq_bits is not the text parser's): next() still returns every record, and says of it whether the filter drops it
	// and under which rule (nte_reads_grammar.h: rp_record_reason; multi-line FASTQ is concatenated first)
	void set_read_filter(const nte_parse::ReadFilter& f) { filter_ = f; }
	unsigned drop_reason() const { return drop_reason_; } // RP_KEPT, RP_DROP_LENGTH or RP_DROP_MEAN_QUAL

  private:
	nte_parse::ReadFilter filter_ = nte_parse::ReadFilter();
	unsigned drop_reason_ = 0;
	unsigned min_qual_ = 0;
	unsigned long long qual_bases_ = 0, masked_bases_ = 0;
	bool fill_();
	int getc_();
	bool getline_(std::string& out, size_t base, bool strip_cr);
	std::string line_;
	void io_loop_();
	void crc_loop_();
	unsigned char* data_(int s) const;
	gzFile f_;
	Gunzip* gz_; // set: the file is a gzip stream inflated by our own decoder (f_ is not used then)
	unsigned char* buf_; // the block being parsed

	int begin_, end_;
	unsigned long long base_, done_; // offset of the first byte read; bytes of the blocks the parser is through with
	unsigned long long limit_, rec_start_, next_start_;
	unsigned long long here_() const { return base_ + done_ + (unsigned long long)begin_; }
	bool eof_;
	int last_char_;
	bool hit_nl_, failed_;
	// blocks are read (and inflated) ahead of the parser by a second thread
	static const int NSLOTS = 4;
	unsigned char* slot_[NSLOTS];
	int slot_len_[NSLOTS];
	bool slot_eof_[NSLOTS];        // the block that marks the end of the input
	bool slot_member_end_[NSLOTS]; // (gz_) the block ends a gzip member whose trailer said slot_crc_ / slot_isize_
	unsigned slot_crc_[NSLOTS], slot_isize_[NSLOTS];
	unsigned long long head_, tail_; // blocks produced / consumed
	unsigned long long crc_done_;    // (gz_) blocks the checksum thread is through with
	int cur_;
	bool stop_;
	bool io_error_ = false; // written by the I/O thread before it publishes the final (empty) block
	std::string io_error_text_;
	std::mutex mu_;
	std::condition_variable cv_;
	std::thread io_;
	std::thread crc_;
};

} // namespace nte_host
