// lio_capi.cpp — the library level of the C-ABI (include/lio_gpu.h): the device count, the last error, the build
// info and the struct sizes the mirrors check themselves against.  There is deliberately no CPU compute path:
// every compute entry point runs the gfx950 kernels or fails with LIO_ERR_NODEV / LIO_ERR_HIP.  The handles are
// in the files beside this one: the online leg's map and scan context in lio_capi_map.cpp, lio_capi_scan.cpp,
// lio_capi_prep.cpp and lio_capi_formats.cpp (lio_capi_online.hpp lists them), the offline leg on a lio_filter in
// lio_capi_post.cpp, the camera leg in lio_capi_camera.cpp, the loop ICP in lio_icp_*.cpp (lio_icp_handle.hpp).
#include "lio_capi_util.hpp"

extern "C" {

int lio_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* lio_last_error(void) { return lio::last_error().c_str(); }

const char* lio_build_info(void) {
    return "lio_gpu: gfx950 HIP kernels (grid kNN + esti_plane + H^T H reduction, ICP); -ffp-contract=off";
}

int lio_abi_struct_sizes(int64_t* out, int n) {
    const int64_t sz[] = {(int64_t)sizeof(lio_map_params),   (int64_t)sizeof(lio_match_params),
                          (int64_t)sizeof(lio_pose),         (int64_t)sizeof(lio_state),
                          (int64_t)sizeof(lio_ieskf_params), (int64_t)sizeof(lio_ieskf_stats),
                          (int64_t)sizeof(lio_icp_params),   (int64_t)sizeof(lio_icp_result),
                          (int64_t)sizeof(lio_localmap),     (int64_t)sizeof(lio_incremental_stats),
                          (int64_t)sizeof(lio_imu_pose),     (int64_t)sizeof(lio_scan_prep_params),
                          (int64_t)sizeof(lio_cloud_field),  (int64_t)sizeof(lio_kernel_timing),
                          (int64_t)sizeof(lio_denoise_params)};
    constexpr int kN = (int)(sizeof(sz) / sizeof(sz[0]));
    if (out)
        for (int i = 0; i < n && i < kN; ++i) out[i] = sz[i];
    return kN;
}

int lio_abi_camera_struct_sizes(int64_t* out, int n) {
    const int64_t sz[] = {(int64_t)sizeof(lio_camera), (int64_t)sizeof(lio_colorize_params)};
    constexpr int kN = (int)(sizeof(sz) / sizeof(sz[0]));
    if (out)
        for (int i = 0; i < n && i < kN; ++i) out[i] = sz[i];
    return kN;
}

int lio_abi_overlay_struct_sizes(int64_t* out, int n) {
    const int64_t sz[] = {(int64_t)sizeof(lio_overlay_params)};
    constexpr int kN = (int)(sizeof(sz) / sizeof(sz[0]));
    if (out)
        for (int i = 0; i < n && i < kN; ++i) out[i] = sz[i];
    return kN;
}

}  // extern "C"
