// What every file with extern "C" entry points (include/speechsplit_amd.h) needs: the refusal path behind ss_last_error(), the
// early-return macros over it and the stream cast.
#pragma once
#include <string>

#include <hip/hip_runtime.h>

namespace ss {

// records m as the calling thread's ss_last_error() and returns -1.  ONE thread-local string for the whole library, defined
// beside ss_last_error in engine.hip: a refusal in any translation unit is read back through the same object.
int fail(const std::string& m);

inline hipStream_t S(void* s) { return (hipStream_t)s; }

}  // namespace ss

#define HIPCHK(x)                                                                      \
    do {                                                                               \
        hipError_t _e = (x);                                                           \
        if (_e != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define CHK(x)                 \
    do {                       \
        int _r = (x);          \
        if (_r != 0) return _r; \
    } while (0)
