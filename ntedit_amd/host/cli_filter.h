// cli_filter.h -- the filter stage of a polishing round: the primary filter (and the secondary one, where the stage makes
// it) into the context, from genome assemblies, from reads, or from a file.
#pragma once

#include "cli_options.h"

#include <string>

namespace nte_cli {

// this round's names of the files the filter stage writes (a round of a cascade has its k in place of {k})
struct RoundNames
{
	std::string hist, save_bf, save_reject_bf;
};

// what the stage leaves for the parameter echo and the polish
struct FilterStage
{
	std::string bf, bfrep;   // the -r and -e names (of a filter that was built: the name its tool would have written it under)
	bool store_held = false; // the resident store stays in HBM while this round polishes (for the next round)
};

// --genome: the filter ntedit-make-genome-bf would write (genome_pass.cpp)
FilterStage filter_from_genome(ntedit_hip_ctx* ctx, const CliOptions& o, const RoundNames& names);
// --reads: the filter ntedit-make-reads-bf would write (reads_build.cpp), and with --reject_cutoff the secondary filter from
// the same pass.  `store_lost`: a cascade's store was released (over its cap, no memory, the polish buffers); no round
// tries it again
FilterStage filter_from_reads(ntedit_hip_ctx* ctx, const CliOptions& o, size_t round, const RoundNames& names, bool* store_lost);
// -r
FilterStage filter_from_file(ntedit_hip_ctx* ctx, const CliOptions& o);

} // namespace nte_cli
