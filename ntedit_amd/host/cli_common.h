// cli_common.h -- what every unit of the `ntedit` binary shares: the program's name, the one way out on an error, a stopwatch.
#pragma once

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <unistd.h>

#define PROGRAM "ntEdit v2.1.1"

namespace nte_cli {

// Prints `head` and the message on stderr, flushes every stream and leaves with status 1 without running destructors: a
// side thread (the pinned pool's, a pipeline stage) may still be running.  Where the run used to end through exit(), after
// its threads were joined, this is observably the same: exit() flushed the streams and nothing else of the process showed.
[[noreturn]] inline void
leave(const char* head, const char* fmt, va_list ap)
{
	fputs(head, stderr);
	vfprintf(stderr, fmt, ap);
	fputc('\n', stderr);
	fflush(nullptr);
	_exit(EXIT_FAILURE);
}

// PROGRAM ": error: <message>\n"
[[noreturn]] __attribute__((format(printf, 1, 2))) inline void
fail(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	leave(PROGRAM ": error: ", fmt, ap);
}

// PROGRAM ": <message>\n": getopt's invalid options (ntedit.cpp:2360-2363) and the lines the library words that way
[[noreturn]] __attribute__((format(printf, 1, 2))) inline void
fail_plain(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	leave(PROGRAM ": ", fmt, ap);
}

// the local time as ctime words it, for the "---------- stage : <date>" lines
inline const char*
now_text()
{
	time_t t;
	time(&t);
	return ctime(&t);
}

class Stopwatch
{
  public:
	void restart() { t0_ = std::chrono::steady_clock::now(); }
	double s() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count(); }
	double ms() const { return 1e3 * s(); }

  private:
	std::chrono::steady_clock::time_point t0_ = std::chrono::steady_clock::now();
};

} // namespace nte_cli
