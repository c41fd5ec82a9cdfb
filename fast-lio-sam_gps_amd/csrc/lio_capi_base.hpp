// lio_capi_base.hpp — the error reporting and the device check of every file behind include/lio_gpu.h: the
// C-ABI files (through lio_capi_util.hpp) and the loop-ICP files (lio_icp_*.cpp), which need none of the filter,
// cluster and camera headers.  Private; each file says `using namespace lio::capi` (or names lio::capi::fail).
// The functions are static: each file has its own and the library exports none.
#pragma once
#include "../../include/lio_gpu.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "lio_error.hpp"

namespace lio::capi {

static inline int fail(int code, const std::string& msg) {
    lio::last_error() = msg;
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(LIO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

static inline int check_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(LIO_ERR_NODEV, "no HIP device visible (this library has no CPU path)");
    if (dev < 0 || dev >= n) return fail(LIO_ERR_ARG, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(LIO_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(LIO_ERR_NODEV, std::string("built for gfx950, device is ") + prop.gcnArchName);
    return LIO_OK;
}

}  // namespace lio::capi
