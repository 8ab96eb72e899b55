// The network plan: everything lp_net_finalize decides on the host before the first byte goes to the device -- the
// architecture bookkeeping, the op list, the buffer list and the packed weight arena.  No HIP header, no HIP call:
// plan.cpp links into a CPU-only program (tests/plan_digest.cpp pins its bytes).  Internal to csrc; the public interface
// is include/litepose_amd.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/litepose_amd.h"

namespace lp_plan {

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_RELU6 = 2 };   // == lp::Act (kernels.h; engine.cpp asserts it)

struct Tensor {
    std::string key;
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool is_set = false;
    bool is_counter = false;      // num_batches_tracked
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

struct Block { int inp, feat, oup, k, stride; bool residual; };
struct Deconv { int refined_in, raw_in, out; };
struct Head { int refined_in, raw_in, oup; };

// OP_DWPW: depthwise + project of an InvBottleneck (fp32 plan); OP_CONVK: dense k x k conv (family 1)
enum OpType { OP_STEM, OP_DW, OP_PW, OP_DECONV, OP_DWPW, OP_CONVK };

// what every op of every plan carries; the walk's site helpers fill all of it but the arena offsets
struct OpBase {
    OpType type = OP_PW;
    std::string name;
    std::string tap;                       // tap name this op's output is published under
    std::string bn0, bn1;                  // the BatchNorm(s) folded into this op, in launch order ("" = none)
    int inA = -1, inB = -1, res = -1, out = -1;   // buffer ids
    int Ca = 0, Cb = 0, Cout = 0, K = 0, S = 1, act = 0;
    int in_div = 1, out_div = 1;           // spatial divisor of the input / output plane
    size_t w_off = 0, b_off = 0;           // float offsets in the weight arena
    size_t st_w0 = 0, st_w1 = 0, st_b1 = 0, st_w2 = 0, st_b2 = 0;   // OP_STEM: the fused stem's copies (conv and depthwise
                                           // tap-major, 1x1 input-major, plain biases; st_b1: 16-bit plan only; 0 = none)
    size_t wrow_off = 0;                   // 7x7 depthwise: pair-interleaved rows [C/2][7][7 taps x 2 ch + 2 pad] (0 = none)
};

// fp32 plan (families 0 and 1)
struct Op : OpBase {
    size_t w2_off = 0, b2_off = 0;         // OP_DWPW: the 1x1 half (w_off/b_off = depthwise half)
    size_t ws_off = 0;                     // exact bf16x3 split of the 1x1 weights (0 = none)
    size_t wdup_off = 0;                   // depthwise weights with every tap stored twice, [C][k*k][2]: the unfused depthwise
                                           // kernels take (w, w) as an aligned 64-bit scalar operand of their packed FMAs
    size_t wpair_off = 0;                  // stride-2 fused block: depthwise weights, channel-pair interleaved [C/2][49][2]
    size_t w3_off = 0, b3_off = 0;         // deconv4: [channel block][parity][channel pair][lane] x 4 taps + bias frags
    size_t w4_off = 0;                     // deconv4x3: [channel block][parity][tap][ks][3 bf16 pieces][lane] x 16 B
    int mid = -1;                          // OP_DWPW: buffer for the depthwise output (fallback only); OP_DECONV: 1 = w2 form
    size_t wk_off = 0;                     // OP_CONVK: bf16x3 A fragments [cout block][tap][ks][3 pieces][lane] x 16 B
    int ups = 0;                           // OP_CONVK: 1 = sources read through a nearest x2 upsample (UpConv)
    bool image_in = false;                 // OP_CONVK: reads the network input (mirrored for the images of a flip pass)
    bool has_bias = true;
    bool fuse_next = false;                // OP_PW expand followed by its OP_DWPW: try mbconv_kernel
};

// 16-bit storage plan (bf16_kernels.hip): the unfused op chain on octet-planar buffers; OP_STEM .. OP_DECONV only
struct BOp : OpBase {
    size_t wt_off = 0;                     // OP_DW 7x7 s1 / 5x5: Toeplitz B fragments for dwt_kernel (0 = none)
    size_t wrow2_off = 0;                  // OP_DW 7x7 s1: the taps as dot2 operands for mbtd_kernel (0 = none)
    bool out_f32 = false;                  // head 1x1: fp32 planar output (d_out0 / d_out1)
};

struct BufferPlan { std::vector<int> ch, div; };   // per buffer: channels, spatial divisor

// the part of lp_net the plan reads and writes (engine.cpp's lp_net derives from it)
struct Net {
    lp_arch arch;
    int c0 = 0;
    std::vector<int> channel;
    std::vector<std::vector<Block>> stages;
    std::vector<Deconv> deconv;
    std::vector<Head> heads;
    std::vector<Tensor> tensors;
    std::map<std::string, int> index;
    int storage = LP_STORAGE_F32;          // the 16-bit formats have their own op list: bops
    bool identity_fold = false;            // calibration's shadow net: bn_fold gives scale 1, shift 0
    // the plan
    std::vector<float> h_packed;
    std::vector<Op> ops;
    std::vector<BOp> bops;
    BufferPlan bufs;
    int out0_buf = -1, out1_buf = -1;
};

// Both return an LP_* code; last_error() is the message of this thread's last refusal.
int init_arch(Net& n, const lp_arch& a);   // channel bookkeeping and the state_dict key table of `a`
int build(Net& n);                         // ops / bops, bufs, h_packed: the form follows arch.family and storage
const char* last_error();

// What lp_net_profile2 reports per launch: the tensors a reference op reads and writes once, its FLOPs, and their depthwise
// / stem-conv share (vector pipe; the rest: matrix cores).  A fused launch costs the sum over the reference ops it replaces.
struct Cost {
    int64_t bytes = 0, flops = 0, flops_valu = 0;
    Cost& operator+=(const Cost& c) { bytes += c.bytes; flops += c.flops; flops_valu += c.flops_valu; return *this; }
};
enum CostPart { COST_OP, COST_DW_HALF, COST_PW_HALF };    // OP_DWPW run as two launches: its depthwise / its 1x1 alone
// one reference op over NB images of H x W.  esz: bytes per stored element (4; 2 for 16-bit storage, out_f32: an fp32 head)
Cost op_cost(const OpBase& o, int esz, bool out_f32, int NB, int H, int W, CostPart part = COST_OP);

size_t arena_push(std::vector<float>& a, size_t count);   // a zeroed 256-byte aligned block; returns its float offset
float round16(int storage, float x);       // x rounded to bf16 / fp16 (nearest even), as fp32

}  // namespace lp_plan
