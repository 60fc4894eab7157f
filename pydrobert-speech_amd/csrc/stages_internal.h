// What the sources of libpds_amd_stages.so share: the calling thread's error string (it lives in sliding.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pds {

// leave `msg` as the calling thread's last error and return PDS_STAGES_ERR_INVALID
int32_t stages_invalid(const char *msg);
// ... "`what`: <HIP's text for err>" and PDS_STAGES_ERR_HIP
int32_t stages_hip_fail(hipError_t err, const char *what);

}  // namespace pds
