// capi_util.h -- error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/rllab_amd.h"

namespace rl {

char* error_buffer();              // thread-local, defined in capi.hip
constexpr int ERROR_BUFFER_LEN = 512;

inline int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), ERROR_BUFFER_LEN, fmt, ap);
    va_end(ap);
    return code;
}

// rl_launch_opts.reserved[] must be zero: a caller that leaves the words uninitialised hears about it at every entry point
// that reads the struct, instead of steering whatever a later version hangs on them.  NULL opts = every field zero.
inline int check_opts(const rl_launch_opts* o, const char* who) {
    if (!o) return 0;
    for (int i = 0; i < (int)(sizeof(o->reserved) / sizeof(o->reserved[0])); ++i)
        if (o->reserved[i] != 0)
            return set_error(RL_ERR_ARG, "%s: rl_launch_opts.reserved[%d] = %d, the reserved words must be zero", who, i,
                             (int)o->reserved[i]);
    return 0;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for a kernel whose dynamic LDS exceeds the 64 KB default, once per
// `done` flag -- a static of the calling template instantiation, so once per process and instantiation.
// (NOT per device: keying the flag by device would be a behaviour change.)
template <class K>
inline int allow_dynamic_lds(K kern, int bytes, bool& done) {
    if (done) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return set_error(RL_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    done = true;
    return 0;
}

// Launch errors (bad configuration, missing code object) surface here without a
// device synchronisation; asynchronous faults surface at the caller's next sync.
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(-3, "%s: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace rl
