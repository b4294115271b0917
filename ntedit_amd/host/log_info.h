// log_info.h -- the console lines the host programs share
#pragma once
#include <cstdio>
#include <ctime>
#include <string>

namespace nte_host {

// btllib::log_info: "[<local time>] [INFO] <msg>" on stderr
inline void
log_info(const std::string& msg)
{
	char ts[64];
	time_t now = time(nullptr);
	strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&now));
	fprintf(stderr, "[%s] [INFO] %s\n", ts, msg.c_str());
}

// the reads filter build's console lines (ntedit_hip_reads_build_args.log)
inline void
reads_log(void*, int to_stdout, const char* line)
{
	if (to_stdout) {
		printf("%s\n", line);
		fflush(stdout);
	} else {
		log_info(line);
	}
}

} // namespace nte_host
