// Launchers of supertrain_kernels.hip (include/litepose_amd.h, "supernet training"); the validation lives in
// supertrain_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/litepose_amd.h"

namespace lp {

// One resize of lp_train_resize: `planes` planes of in x in cells -> out x out (kind 0, fp32), or `planes` (index, flag)
// pairs of a joints tensor (kind 1, int32).
struct ResizeJob {
    const void* src;
    void* dst;
    int32_t planes, in, out, kind;
};
struct ResizeJobs {
    ResizeJob job[7];          // the images, then per stage heatmaps, masks, joints
    int32_t njobs, S, B;
};

int64_t resize_job_threads(const ResizeJob& j);
void launch_subnet_gather(const lp_subnet_desc* desc, int count, float* sub, int64_t sub_elems, hipStream_t s);
void launch_subnet_scatter(const lp_subnet_desc* desc, int count, const float* gsub, int64_t sub_elems, float* full,
                           int64_t full_elems, hipStream_t s);
void launch_train_resize(const ResizeJobs& jobs, hipStream_t s);

}  // namespace lp
