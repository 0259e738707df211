// The error core of a satellite library (libb2s_vocoder.so, libb2s_metrics.so, libb2s_mcd.so, libb2s_f0.so, libb2s_dur.so,
// libb2s_pros.so, libb2s_va.so, libb2s_vp.so).  side_common.hip is compiled into each of them (build.sh), so each has a thread-local message slot of its own behind its b2s_*_last_error(); everything here has
// hidden visibility and stays out of the dynamic symbol tables.
#pragma once
#include <cstddef>

namespace b2s_side {

// formats the message (at most 511 bytes) into this library's slot of the calling thread, and returns 1
__attribute__((visibility("hidden"), format(printf, 1, 2))) int fail(const char *fmt, ...);
// what the library's b2s_*_last_error() returns
__attribute__((visibility("hidden"))) const char *last_error();
// after the launches of an entry point: 0, or fail("<what>: launch failed: <hip string>")
__attribute__((visibility("hidden"))) int launch_status(const char *what);
// workspace regions start at multiples of 256 bytes
constexpr size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace b2s_side
