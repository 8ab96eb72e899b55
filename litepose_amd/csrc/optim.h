// One argument chunk of the optimizer launches (optim_api.cpp packs it, optim_kernels.hip takes it by value).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/litepose_amd.h"

namespace lp {

constexpr int OPTIM_THREADS = 256;

// tensors [first, first + tensors) of the call's list, consecutive; ptr[k][t]: param, grad, exp_avg | momentum buffer,
// exp_avg_sq of tensor first + t (unused rows stay NULL); map[b] = t << 24 | block index inside the tensor (a tensor has at
// most 2^31 / LP_OPTIM_BLOCK_ELEMS = 2^19 blocks, a chunk at most 64 tensors).  With the scalars of a launch the whole
// argument block stays within 4 KB.
struct OptimChunk {
    float* ptr[4][LP_OPTIM_CHUNK_TENSORS];
    int32_t numel[LP_OPTIM_CHUNK_TENSORS];
    uint32_t map[LP_OPTIM_CHUNK_BLOCKS];
    int32_t first, tensors, blocks, reserved;
};
static_assert(sizeof(OptimChunk) + 6 * 8 <= 4096, "an optimizer launch's arguments must fit 4 KB");
static_assert(LP_OPTIM_BLOCK_ELEMS % (4 * OPTIM_THREADS) == 0 && LP_OPTIM_CHUNK_TENSORS <= 256, "chunk geometry");

void launch_adam_chunk(const OptimChunk& ck, const float* step, const double* lr, double beta1, double beta2, double eps,
                       double weight_decay, hipStream_t s);
void launch_step_advance(float* step, int count, hipStream_t s);
void launch_sgd_chunk(const OptimChunk& ck, bool with_momentum, const double* lr, double momentum, double weight_decay,
                      int nesterov, hipStream_t s);

}  // namespace lp
