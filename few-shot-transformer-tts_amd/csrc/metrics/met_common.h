// Shared by the sources of libb2s_metrics.so: the error slot behind b2s_met_last_error() (defined in dtw.hip, thread-local).
#ifndef B2S_MET_COMMON_H
#define B2S_MET_COMMON_H

namespace b2s_met {

// formats the message into the calling thread's error slot and returns 1 (not exported from the library)
__attribute__((visibility("hidden"), format(printf, 1, 2))) int fail(const char *fmt, ...);

}  // namespace b2s_met
#endif
