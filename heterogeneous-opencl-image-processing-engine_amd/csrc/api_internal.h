// api_internal.h — internal: what the files that implement the C ABI (mi_blur_api.cpp, comm_api.cpp, table_api.cpp) share.
#pragma once
#include "../../include/mi_blur.h"

#include <hip/hip_runtime.h>

// A failed HIP call ends the export with its status; the runtime's sticky last error is cleared.
#define HIP_TRY(expr)                                                       \
    do {                                                                    \
        hipError_t e_ = (expr);                                             \
        if (e_ != hipSuccess) { (void)hipGetLastError(); return MI_BLUR_ERR_HIP_BASE - (int)e_; } \
    } while (0)
