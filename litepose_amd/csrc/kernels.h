// Internal launch interface between the host engine (engine.cpp) and the gfx950
// kernels (net_kernels.hip, ae_kernels.hip).  Not part of the public C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lp {

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_RELU6 = 2 };

// A kernel variant whose registers spill to scratch (private segment) is kept OFF the path (a performance rule: a spill in
// a depthwise loop costs more than the fusion saves), and since round 4 no variant of the build spills at all
// (tests/test_host_cpu.py checks the build's resource report).  History: round 3 refused spilling variants because wrong
// batches went away with them (109 / 30 000 -> 0 / 40 000); round 4 found the cause of those batches elsewhere -- the
// packed-fp32 op_sel erratum, DESIGN 5b -- and the spilling variants had merely changed which kernels shared a CU.
// Every fused-block launcher still asks this before it picks a variant and falls through to the next form.
bool uses_scratch(const void* kernel_fn);

// The launch gate of every kernel that takes dynamic LDS: false when the kernel needs scratch (above), otherwise
// kernel_allow_lds.  A launcher that returns bool returns false on it (its caller takes the next form).
bool kernel_ready(const void* kernel_fn, size_t dyn_lds);
// Raises the kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) to dyn_lds on the current device:
// one runtime call per (device, kernel) and thread, a table lookup afterwards (eager and capture launches; a graph replay
// runs no launcher).  false = the runtime refused, the sticky error is cleared.  Alone it serves the void launchers that have no other form to fall
// back to (peaks_topk*, refine_mid_kernel): they launch anyway and the launch error surfaces at the end of the call.
bool kernel_allow_lds(const void* kernel_fn, size_t dyn_lds);

// name of the kernel the last launch_* call enqueued (profiling aid, set by the launchers)
extern thread_local const char* last_kernel_tag;

// geometry of the last network launch (round 6: lp_net_profile_launches -> bench.py's `cus_occupied`): workgroups of the
// grid, threads per workgroup, dynamic LDS, and how many such workgroups the occupancy query admits per CU.  Filled only
// while a handle profiles (launch_notes: the occupancy query is a host call per launch).
struct LaunchNote { int grid = 0, block = 0, lds = 0, wgs_per_cu = 0; };
extern thread_local LaunchNote last_launch;
extern thread_local bool launch_notes;
void note_launch(const void* fn, dim3 grid, dim3 block, size_t lds);
#define LP_LAUNCH(kern, grid, block, lds, stream, ...)                                                   \
    do {                                                                                                 \
        if (lp::launch_notes) lp::note_launch(reinterpret_cast<const void*>(kern), grid, block, lds);    \
        hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                 \
    } while (0)

// -DLP_CLAIM_CU (the `regstage` flavour): a fused-block workgroup (8 waves, launch_bounds(512, 2)) that claims the whole
// 256-register budget fills the register file of all four SIMDs of its CU, so no wave of another kernel is resident
// next to it -- round 3's mitigation of the rare wrong batch, a side effect on WHERE the victims of the erratum ran, not a
// cure.  Off in the library: co-residency is what the two-network schedule lives on.
#ifdef LP_CLAIM_CU
#define LP_OWN_CU() asm volatile("; own the CU: whole register budget, no co-resident waves" ::: "v255")
#else
#define LP_OWN_CU() ((void)0)
#endif

// ---- network (planar NCHW fp32) --------------------------------------------------
// stem: conv3x3 s2 p1 (3 -> 32) + folded BN + ReLU6.  w [32][27] (ci,ky,kx), b [32].
// flip_from: images with index >= flip_from read x mirrored along W (TTA pass).
void launch_stem(const float* x, const float* w, const float* b, float* out,
                 int N, int H, int W, int flip_from, int x_batch, hipStream_t s);

// the whole stem (conv3x3 s2 + dw3x3 + 1x1, stem_kernels.hip) in one launch; weights tap-/input-major:
// w0t [27][32], w1t [9][32], w2t [32][c0].  false = shape not supported -> the three kernels below
bool launch_stem3(const float* x, const float* w0t, const float* b0, const float* w1t, const float* b1,
                  const float* w2t, const float* b2, float* out, int N, int H, int W, int c0, int flip_from,
                  int x_batch, hipStream_t s);

// bf16 storage (round 6): the same launch with bf16-rounded weights (fp32 arrays in the layouts above), every tensor the
// stemb / dwb<3,1> / pwb chain stores rounded at the same place, output as octet-planar bf16 records
bool launch_stem3b(const float* x, const float* w0t, const float* b0, const float* w1t, const float* b1,
                   const float* w2t, const float* b2, void* out, int N, int H, int W, int c0, int flip_from,
                   int x_batch, hipStream_t s, bool f16 = false);

// depthwise KxK, stride S, pad K/2, + bias + act.  w [C][K*K], wdup [C][K*K][2] (every tap twice: the stride-1 kernels
// take (w, w) as an aligned scalar pair of their packed FMAs, engine.cpp pack_dw_dup), b [C].
void launch_dw(const float* in, const float* w, const float* wdup, const float* b, float* out,
               int N, int C, int H, int W, int K, int S, int act, hipStream_t s);

// pointwise 1x1 over up to two channel-concatenated sources (fp32 MFMA 32x32x2):
//   out[n][co][p] = act( sum_k Wp[co][k] * src[k][p] + b[co] ) (+ res[n][co][p])
// wp: packed A fragments [ceil(Cout/32)][K/2][64], K = Ca + Cb (even).
void launch_pw(const float* inA, int Ca, const float* inB, int Cb,
               const float* wp, const float* b, const float* res, float* out,
               int N, int HW, int Cout, int act, hipStream_t s, const void* wsplit = nullptr, int pw3d_mode = 1);
// wsplit: optional exact bf16x3 split of the same weights ([Cout/32][K/16][3][64 lanes] x 4 dwords) for
// the compute-bound variant; only used for single-source layers with K % 16 == 0
// the pw2_kernel<NB, PXV> launch_pw picks when it does not take the wsplit route (host arithmetic, no launch)
struct PwTile { int NB, PXV; };
PwTile pw_tile_choice(int N, int Ca, int Cb, int Cout, int HW, bool has_res);

// fused depthwise(K7)+bias+ReLU6 -> 1x1 project + bias (+res); false = shape not supported
bool launch_dwpw(const float* in, const float* wdw, const float* bdw, const float* wp, const float* bias,
                 const float* res, float* out, int N, int C, int H, int W, int K, int S, int Cout,
                 hipStream_t s, int diag = 0);
// diagnostics of option "diag_dwpw" (DESIGN 5b): events logged by the self-checking bias fetch; returns their number
int dwpw_diag_read(unsigned* host, int cap_words, bool clear);

// fused output head: relu(dw5(refined)+b) and relu(dw5(raw)+b) -> dual-source 1x1 (wp = pack_pw A fragments over the
// concatenated channels, no bias) in one launch; false = shape not supported -> dw + dw + pw
// wpairA / wpairB: depthwise taps + bias of each source, channel-pair interleaved [C/2][K*K + 1][2]
// inB = wpairB = nullptr, Cb = 0: the one-source head of a plain_head net (pose_simplenet), bit-identical to dw + pw
bool launch_headfuse(const float* inA, int Ca, const float* inB, int Cb, const float* wpairA, const float* wpairB,
                     const float* wp, float* out, int N, int H, int W, int K, int Cout, hipStream_t s);

// whole InvBottleneck (stride 1, k7, Cin/Cout <= 32) in one kernel; false = not supported -> unfused
bool launch_mbconv(const float* x, const float* w1p, const float* b1f, const float* wdw,
                   const float* bdw, const float* w2p, const float* b2f, const float* res, float* out,
                   int N, int Cin, int Cexp, int Cout, int H, int W, int K, int S, hipStream_t s,
                   const float* wdw_pair = nullptr, const void* w1_split = nullptr, const void* wdw_rows = nullptr,
                   int mbconv2 = 1);
// Cin = 24: mbconv_kernel / mbconv_s2_kernel (w1p, wdw_pair, bdw).  Cin = 16, stride 1: mbconv2_kernel, which takes
// wdw_rows: depthwise weights as pair rows [C/2][7][7 taps x 2 ch + bias pair in row 0's pad], and
// w1_split: exact bf16x3 split of the expand weights (pack_pw): its expand runs on bf16 MFMAs

// whole InvBottlenecks (stride 1, k7) on a 16x16 plane, one workgroup per image, bf16x3 MFMA 1x1s (mb16_kernels.hip):
// a RUN of up to MB16_MAX_RUN consecutive blocks per launch.  Per block: w1s / b1f / w2s / b2f = the exact bf16x3
// weight splits and D-fragment biases pw3_kernel uses, wrow = depthwise filter rows [C/2][7][7 taps x 2 ch, bias pair
// in row 0's pad], out = the block's output tensor (every block stores it).  res: every block adds its input
// (Cin == Cout; a run of more than one block is residual blocks of ONE shape); !res: one block.
constexpr int MB16_MAX_RUN = 10;
struct Mb16Run {
    const void* w1s[MB16_MAX_RUN];
    const float* b1f[MB16_MAX_RUN];
    const void* wrow[MB16_MAX_RUN];
    const void* w2s[MB16_MAX_RUN];
    const float* b2f[MB16_MAX_RUN];
    float* out[MB16_MAX_RUN];
    int nblocks;
};
bool mb16_supported(int Cin, int Cexp, int Cout, int H, int W, int K, int S, bool res);
bool launch_mb16(const float* x, const Mb16Run& run, bool res, int N, int Cin, int Cexp, int Cout, int H, int W,
                 int K, int S, hipStream_t s);

// whole InvBottleneck (stride 1, k7, Cin % 16 == 0, Cin <= 48, Cout <= 64) on 16x16 output tiles of a larger plane,
// one 8-wave workgroup per tile, both 1x1 on bf16x3 MFMAs, px-split projection (mbtile_kernels.hip); same packed
// weights as launch_mb16 (w1s / b1f / wrow / w2s / b2f).  false = shape not supported / switched off (options "mbt" / "mbt_s2")
// mode_strip = option "mbt_strip": planes with W == 32 as 32-wide x 16-row strips (the same kernel name and results)
bool launch_mbt(const float* x, const void* w1s, const float* b1f, const void* wrow, const void* w2s,
                const float* b2f, const float* res, float* out, int N, int Cin, int Cexp, int Cout, int H, int W,
                int K, int S, hipStream_t s, int mode = 1, int mode_s2 = 1, int mode_strip = 1);
// Host arithmetic only: launch_mbt's one source of the form, and what lp_mbt_form reports.  kind: the kernel body
// (MBT_TILE = mbt_kernel<CK, NMT, RES>, MBT_STRIP = mbt_kernel<CK, NMT, RES, 16>, MBT_S2 = mbt_s2_kernel<CK, NMT>), or
// MBT_NONE: launch_mbt returns false.  has_res: the block adds its input (launch_mbt: res == x).  cus: the CU count the
// default rule of mode_strip = 1 compares with; <= 0 asks the device.  The form is the one BEFORE the uses_scratch checks,
// which need a device: launch_mbt turns a strip whose kernel needs scratch into the tile of the same CK, NMT, RES, and
// refuses a tile or an s2 form that does.
enum MbtKind { MBT_NONE = 0, MBT_TILE = 1, MBT_STRIP = 2, MBT_S2 = 3 };
struct MbtForm { int kind = MBT_NONE, CK = 0, NMT = 0; bool RES = false; };
MbtForm mbt_form(int N, int Cin, int Cexp, int Cout, int H, int W, int K, int S, bool has_res, int mode, int mode_s2,
                 int mode_strip, int cus);

// fused pair of ConvTranspose2d(k4,s2,p1) + add + folded BN + ReLU.
// w [Ca+Cb][Cout][4][4] (BN scale folded), b [Cout].  in: [N,C,h,w] -> out [N,Cout,2h,2w]
// Every deconv launcher (and launch_deconvb): inB = nullptr, Cb = 0 runs the one-source form (plain_head: ConvT(refined))
void launch_deconv_pair(const float* inA, int Ca, const float* inB, int Cb,
                        const float* w, const float* b, float* out,
                        int N, int h, int w_, int Cout, hipStream_t s);

// MFMA form (Cout <= 32): wp = per-parity A fragments [4][2*(Ca+Cb)][64], bias in D-fragment order
void launch_deconv4(const float* inA, int Ca, const float* inB, int Cb, const float* wq, const float* bias,
                    float* out, int N, int h, int w_, int Cout, hipStream_t s);
// the same on the exact bf16x3 split: ws = [block][parity][tap][ceil(Ct/16)][3 pieces][64 lanes] x 16 B
// (false = shape not supported / disabled -> launch_deconv4)
bool launch_deconv4x3(const float* inA, int Ca, const float* inB, int Cb, const void* ws, const float* bias,
                      float* out, int N, int h, int w_, int Cout, hipStream_t s);
void launch_deconv_mfma(const float* inA, int Ca, const float* inB, int Cb, const float* wp,
                        const float* bias, float* out, int N, int h, int w_, int Cout, hipStream_t s);

// dense KxK convolution (K 3/5/7, stride S 1/2, pad K/2) over up to two channel-concatenated sources + bias + act on the
// exact bf16x3 split (convk_kernels.hip; the pose_resnet family).  in: [N,C,IH,IW]; ups = 1: read through a nearest x2
// upsample (UpConv: the conv runs on the 2IH x 2IW plane, its zero padding included).  ws = pack_convk's A fragments
// [ceil(Cout/32)][K*K][ceil((Ca+Cb)/16)][3 pieces][64 lanes] x 16 B, bias [Cout].  Images >= flip_from read source A
// mirrored along W, image n of source A is n % x_batch (the first conv of a TTA pass).  false = shape not supported
bool launch_convk3(const float* inA, int Ca, const float* inB, int Cb, const void* ws, const float* bias, float* out,
                   int N, int IH, int IW, int K, int S, int ups, int Cout, int act, int flip_from, int x_batch,
                   hipStream_t s);

// ---- BatchNorm re-calibration (training-mode forward of a supernet sub-network, calib_kernels.hip) ----
// raw forms of the two convolutions whose library kernels have their activation built in: the stem conv (w [32][27]) and
// the pair of ConvTranspose2d(k4,s2,p1) (w [Ca+Cb][Cout][4][4]; inB = nullptr: one source), no bias, no activation
void launch_stem_raw(const float* x, const float* w, float* out, int N, int H, int W, hipStream_t s);
void launch_deconv_raw(const float* inA, int Ca, const float* inB, int Cb, const float* w, float* out, int N, int h,
                       int w_, int Cout, hipStream_t s);
// batch statistics of x [N,C,HW]: per-channel partial (sum, sum of squares) pairs in fp64 -> part
// (bn_partial_doubles(N, C, HW) doubles, 16-byte aligned), one per workgroup, combined by launch_bn_apply in index order
struct BnCut { int S, chunk, vec; };     // S slices of `chunk` units (float4s when vec, else floats) per channel: grid (S, C)
BnCut bn_cut(int N, int C, int HW);
size_t bn_partial_doubles(int N, int C, int HW);
void launch_bn_stats(const float* x, double* part, int N, int C, int HW, hipStream_t s);
// in place: x = act((x - mean) * rsqrt(var + eps) * gamma + beta) (+ res) with the batch's mean / biased variance, and
// running = (1 - momentum) * running + momentum * batch (unbiased variance).  bn = [gamma | beta | mean | var] x C (device)
void launch_bn_apply(float* x, const float* res, const double* part, float* bn, int N, int C, int HW, int act,
                     double momentum, double eps, hipStream_t s);

// ---- network, 16-bit storage (octet-planar [N][C/8][HW][8] bf16 or fp16; bf16_kernels.hip, mbtile_bf16.hip) ----
// Every launcher below takes the storage format last: f16 = false (default) runs the kernels' lp::Bf16 instances, true their
// lp::F16 (IEEE half) ones -- one template per kernel with the format as its leading argument, chosen by with_fmt
// (fmt16.h): same template lists, same shape rules, same refusals, same last_kernel_tag.
// The weight arrays hold values rounded to the launch's format (engine.cpp rne16).
// stem on the fp32 image; w [32][27] fp32 (bf16-rounded values), b [32]
void launch_stemb(const float* x, const float* w, const float* b, void* out, int N, int H, int W, int flip_from,
                  int x_batch, hipStream_t s, bool f16 = false);
// depthwise; w [C/8][K*K + 1][8] fp32: taps (bf16-rounded values), then the bias octet.  false = not supported
// depthwise 7x7 / 5x5 stride 1 as banded matrix products on v_mfma_f32_16x16x32_bf16 (option "dwt": 0 never, 1 the 7x7
// ones, 2 (default) also the heads' 5x5).
// wt: Toeplitz B fragments [C][K filter rows][64 lanes] x 16 B (pack_dwt); wb: the octet taps + bias array of dwb
bool launch_dwt(const void* in, const void* wt, const float* wb, void* out, int N, int C, int H, int W, int K, int act,
                hipStream_t s, bool f16 = false);
bool launch_dwb(const void* in, const float* w, void* out, int N, int C, int H, int W, int K, int S, int act,
                hipStream_t s, bool f16 = false);
// 1x1 over up to two octet sources; wf = bf16 A fragments [ceil(Cout/32)][ceil((Ca+Cb)/16)][64 lanes] x 16 B,
// bias in D-fragment order [ceil(Cout/32)][2][16]; out: octet bf16 (res: same layout) or fp32 planar (out_f32)
bool launch_pwb(const void* inA, int Ca, const void* inB, int Cb, const void* wf, const float* bias, const void* res,
                void* out, int N, int HW, int Cout, int act, bool out_f32, hipStream_t s, bool f16 = false);
// an output head of the bf16-storage network in one launch (round 6; bf16_kernels.hip): dwt_kernel<5> on both sources + the
// dual-source 1x1 with fp32 planar output; wtA / wbA, wtB / wbB = the two depthwise ops' dwt fragments and tap / bias blocks, wf =
// pwb's A fragments of the head's 1x1.  false = shape not taken (Cout > 32, small planes) -> the three launches
// inB = wtB = wbB = nullptr, Cb = 0: the one-source head of a plain_head net (dwt<5> + pwb in one launch, the same bits)
bool launch_headb(const void* inA, int Ca, const void* inB, int Cb, const void* wtA, const float* wbA, const void* wtB,
                  const float* wbB, const void* wf, float* out, int N, int H, int W, int K, int Cout, hipStream_t s,
                  bool f16 = false);
// whole 7x7 InvBottleneck (stride 1: mbtb_kernel; stride 2: mbtb_s2_kernel) on octet records in one launch
// (mbtile_bf16.hip): w1 / b1f and w2 / b2f are the expand's and the project's pwb arrays, wrow = pack_wrow_b's filter
// rows; res = x or null; H, W = the INPUT plane.  false = shape not taken (the caller runs the pwb / dwt|dwb / pwb
// chain), or switched off (options "mbtb" / "mbtb_s2").
bool launch_mbtb(const void* x, const void* w1, const float* b1f, const void* wrow, const void* w2, const float* b2f,
                 const void* res, void* out, int N, int Cin, int Cexp, int Cout, int H, int W, int K, int S,
                 hipStream_t s, int mode = 1, int mode_s2 = 1, const void* wrow2 = nullptr, int mode_d = 1,
                 bool f16 = false);
// phase trace of mbtb_kernel / mbtd_kernel (`trace` flavour; mbtile_bf16.hip): 64 words per workgroup
// (8 waves x 8 slots) of the launches selected by wg_trace_read; -2 = not in this library
int phase_trace_read(unsigned long long* host, int nwg);
// workgroup timeline (`trace` flavour): copies 4 words per workgroup of the selected launches, then selects Cexp = sel
int wg_trace_read(unsigned long long* host, int nwg, int sel);
// fused pair of ConvTranspose2d(k4,s2,p1) + add + BN + ReLU; wf [block][parity][tap][ks][64 lanes] x 16 B
bool launch_deconvb(const void* inA, int Ca, const void* inB, int Cb, const void* wf, const float* bias, void* out,
                    int N, int h, int w_, int Cout, hipStream_t s, bool f16 = false);
void launch_octet_to_planar(const void* in, float* out, int N, int C, int HW, hipStream_t s, bool f16 = false);

// ---- associative-embedding post-process -------------------------------------------
struct ParseParams {
    int J, M;
    double det_thr, tag_thr;            // the reference compares float64 (group.py:38-41,82)
    int use_det_val, ignore_too_much, nms_k, tag_per_joint;
    int joint_order[32];
};

struct FlipIndex { int v[32]; };
// stage merge at the stage-1 resolution (inference.py:84-146): writes
// mid [N][4][J][h1][w1] = {heat, heat_flip, tag, tag_flip}
// add0 / add1 / add0f / add1f: optional additive maps of the output shapes, added as the outputs are read (exact x2
// stage merge only: false = not available for this shape, nothing launched)
bool launch_tta_stage(const float* out0, const float* out1, const float* out0f, const float* out1f,
                      int N, int J, int C0, int C1, int tag_off, int h0, int w0, int h1, int w1,
                      const FlipIndex& flip_index, float* mid, hipStream_t s, const float* add0 = nullptr,
                      const float* add1 = nullptr, const float* add0f = nullptr, const float* add1f = nullptr);
void launch_maps_accumulate(float* acc, const float* src, long count, hipStream_t s);
// tag == nullptr: det only (exact x2 projection only; false = not available for this shape)
bool launch_tta_project(const float* mid, int N, int J, int h1, int w1, int Hp, int Wp, int T,
                        float* det, float* tag, hipStream_t s);
// one scale of launch_tta_merge_scales: the layout of lp_scale_mid (include/litepose_amd.h)
constexpr int MAX_SCALES = 8;
struct ScaleMid {
    const float* mid;       // [N][4][J][h1][w1] of lp_tta_stage
    int h1, w1;
};
static_assert(sizeof(ScaleMid) == 16, "ScaleMid must match lp_scale_mid (16 bytes)");
struct ScaleTable { ScaleMid s[MAX_SCALES]; };      // passed by value: a captured launch holds the table itself
// multi-scale aggregation of S stage merges (descending scale order) into det [N,J,Hf,Wf] / tag [N,J,Hf,Wf,T]
void launch_tta_merge_scales(const ScaleTable& t, int S, int first_unit, int N, int J, int T, int project2image,
                             int Hf, int Wf, float* det, float* tag, hipStream_t s);

// tag == nullptr: the winners' tags are the exact x2 projection of `mid` (lp_parse_dm); false = not available
bool launch_peaks_topk(const float* det, const float* tag, int N, int J, int H, int W, int T,
                       const ParseParams& p, float* val_k, int* ind_k, float* tag_k, hipStream_t s,
                       const float* mid = nullptr);
void launch_group(const float* val_k, const int* ind_k, const float* tag_k, int N, int W, int T,
                  const ParseParams& p, int pcap, float* ans, int* count, hipStream_t s);
// prev [N][pcap][4] mean tag of detected joints, miss [N][pcap] bitmask of joints to refine
void launch_adjust_scores(const float* det, const float* tag, int N, int J, int H, int W, int T,
                          int pcap, int do_adjust, float* ans, const int* count, float* scores,
                          float* prev, unsigned* miss, hipStream_t s);
void launch_refine(const float* det, const float* tag, int N, int J, int H, int W, int T, int pcap,
                   float* ans, const int* count, const float* prev, const unsigned* miss,
                   hipStream_t s);
// refine with det from HBM and the tags evaluated from `mid` (the tag tensor is never materialised)
bool launch_refine_dm(const float* det, const float* mid, int N, int J, int h1, int w1, int T, int pcap, float* ans,
                      const int* count, const float* prev, const unsigned* miss, hipStream_t s);
// the same three steps straight from the stage-1-resolution merge `mid` (exact x2 projection): the full-resolution
// det / tag maps are never materialised (ae_mid_kernels.hip).  launch_peaks_topk_mid: false = shape not supported
// round 5: the register column walk straight from mid (ae_kernels.hip peaks_topk_walk_kernel): w1 even; false = not supported
bool launch_peaks_topk_walk(const float* mid, int N, int J, int h1, int w1, int T, const ParseParams& p,
                            float* val_k, int* ind_k, float* tag_k, hipStream_t s);
bool launch_peaks_topk_mid(const float* mid, int N, int J, int h1, int w1, int T, const ParseParams& p,
                           float* val_k, int* ind_k, float* tag_k, hipStream_t s);
void launch_adjust_scores_mid(const float* mid, int N, int J, int h1, int w1, int T, int pcap, int do_adjust,
                              float* ans, const int* count, float* scores, float* prev, unsigned* miss,
                              hipStream_t s);
void launch_refine_mid(const float* mid, int N, int J, int h1, int w1, int T, int pcap, float* ans,
                       const int* count, const float* prev, const unsigned* miss, hipStream_t s);
void launch_warp_affine_norm(const unsigned char* src, int H, int W, int Hd, int Wd, const double* minv,
                             const float* mean, const float* sd, unsigned char* dst_u8, float* dst_f32,
                             hipStream_t s, int nimg = 1);      // nimg images [nimg,H,W,3] -> [nimg,...], one transform
void launch_final_preds(float* ans, const int* count, int N, int pcap, int J, int T,
                        double sx, double tx, double sy, double ty, hipStream_t s);
// per-image source / transform of launch_warp_affine_norm_v: the layout of lp_warp_desc (include/litepose_amd.h)
struct WarpDesc {
    long long src_offset;   // byte offset of the [H,W,3] uint8 source in the packed buffer
    int H, W;
    double minv[6];         // inverted (dst -> src) 2x3 matrix
};
static_assert(sizeof(WarpDesc) == 64, "WarpDesc must match lp_warp_desc (64 bytes)");
void launch_warp_affine_norm_v(const unsigned char* src, long long src_bytes, const WarpDesc* desc, int N, int Hd,
                               int Wd, const float* mean, const float* sd, unsigned char* dst_u8, float* dst_f32,
                               hipStream_t s);      // N images of their own sizes / transforms -> [N,...] at (Hd, Wd)
void launch_final_preds_v(float* ans, const int* count, int N, int pcap, int J, int T, const double* coef,
                          hipStream_t s);           // coef [N,4] = (sx, tx, sy, ty) per image, device
// per-image source / transform / mirror of launch_warp_affine_flip_norm_v: the layout of lp_aug_desc
struct AugDesc {
    long long src_offset;   // as WarpDesc
    int H, W;
    double minv[6];
    int flip, reserved;     // flip != 0: output column x takes warped column Wd - 1 - x; reserved must be 0
};
static_assert(sizeof(AugDesc) == 72, "AugDesc must match lp_aug_desc (72 bytes)");
void launch_warp_affine_flip_norm_v(const unsigned char* src, long long src_bytes, const AugDesc* desc, int N, int Hd,
                                    int Wd, const float* mean, const float* sd, unsigned char* dst_u8, float* dst_f32,
                                    hipStream_t s);  // the train loader's image side: warp, mirror, ToTensor + Normalize

// ---- the reference's real-time parser (nano_demo/fast_utils; fast_kernels.hip) ------
// find_peaks: the first M peaks of every plane in raster order; tmap is read at (plane * H * W + y * W + x) * tstride
// (W <= 1024, window odd <= 7, M <= 10: checked by the caller)
void launch_fast_peaks(const float* det, const float* tmap, long tstride, int N, int J, int H, int W, float threshold,
                       int window, int M, int* count, float* val, float* tag, int* ind, hipStream_t s);
// assign: joint_order = J host ints (a permutation of 0..J-1), copied into the launch's arguments
void launch_fast_assign(const int* count, const float* val, const float* tag, const int* ind, int N, int J, int M,
                        const int* joint_order, float tag_threshold, float* ans, int* num, hipStream_t s);

// ---- COCO keypoint evaluation: OKS + greedy matching per record row (eval_kernels.hip) ------
// the host tables of lp_kpt_eval, copied into the launch: vars[j] = (2 sigma_j)^2, and per result bit b = a * n_thr + t
// the starting bound min(thr[t], 1 - 1e-10) and the area range [lo, hi] of a
struct KptEvalTables {
    double vars[32];
    double best0[32];
    double lo[32];
    double hi[32];
};
// one workgroup per row; max_dets <= 32, nbits <= 32, J_eval <= min(J, 32): checked by the caller.  An image's
// annotations beyond the 64th are not read.
void launch_kpt_eval(const float* ans, const int* count, const float* scores, int N, int pcap, int J, int T, int J_eval,
                     const int* row_image, const double* gt_kpts, const double* gt_area, const double* gt_bbox,
                     const int* gt_flags, const int* gt_first, int images, const KptEvalTables& tb, int nbits,
                     int max_dets, float* score_out, int* num_out, int* src_out, unsigned* match_out,
                     unsigned* ignore_out, double* oks_out, hipStream_t s);

// ---- utils.vis: skeletons drawn into uint8 HWC images (vis_kernels.hip; the raster rule is DESIGN.md 4c) ------
struct ImageDesc {                          // lp_image_desc (include/litepose_amd.h)
    long long offset;
    int H, W;
};
struct VisTables {                          // the link table and the palette, passed to the kernel by value
    unsigned char la[64], lb[64];           // link l joins joints la[l] and lb[l] (an index >= J: skipped)
    unsigned char pal[96];                  // 32 colours of 3 bytes
};
constexpr int VIS_PASS_PRIMS = 512;         // primitives resolved per pass into the 8 KB LDS table of a workgroup
// desc == nullptr: N images [N,H,W,3]; otherwise N images at desc[n] inside images[0, bytes).  links: n_links host pairs,
// palette: n_colors host byte triples, both copied into the launch's arguments.  Sizes are checked by the caller.
void launch_draw_poses(unsigned char* images, long long bytes, const ImageDesc* desc, int N, int H, int W,
                       const float* kpts, const int* count, int pcap, int J, int D, const int* links, int n_links,
                       const unsigned char* palette, int n_colors, int Rj, int Rl, hipStream_t s);

// ---- training targets and loss (target_kernels.hip, loss_kernels.hip; lp_target_maps / lp_target_masks / lp_pose_loss) ------
struct TargetDesc {                         // lp_target_desc (include/litepose_amd.h)
    double mat[6];                          // FORWARD (src -> output plane) 2x3 matrix
    int flip, reserved;
};
static_assert(sizeof(TargetDesc) == 56, "TargetDesc must match lp_target_desc (56 bytes)");
struct TargetFlip { int idx[32]; };         // flip_index, passed to the kernel by value (entries in [0, J): checked by the caller)
// one launch; heat [N,J,R,R] and / or jout [N,M,J,2]; J <= 32, M <= 64, side = 2 * s3 + 3: checked by the caller
void launch_target_maps(const double* joints, long P_tot, const int* first, const TargetDesc* desc, int N, int J, int R,
                        const TargetFlip& fi, const float* gauss, int side, int s3, int M, int tag_per_joint, float* heat,
                        int* jout, hipStream_t s);
// one launch; out [N,R,R]; src may be null when src_bytes is 0 (every usable row is then an all-ones one)
void launch_target_masks(const unsigned char* src, long long src_bytes, const AugDesc* desc, int N, int R, float* out,
                         hipStream_t s);
constexpr int LOSS_STRIP = 4096;            // floats of a plane per workgroup (and per fp64 partial) of the heatmap loss
// partial [N * J * S] fp64, S = ceil(R * R / LOSS_STRIP)
void launch_heat_partial(const float* pred, const float* gt, const float* mask, int N, int C, int J, int R, int S,
                         double* partial, hipStream_t s);
// partial == nullptr: no heatmap term (heat_loss untouched); tag_offset < 0: no tag terms (push_out / pull_out untouched)
void launch_loss_finish(const double* partial, int N, int JS, double heat_count, double heat_factor, const float* out,
                        int C, int R, int tag_offset, const int* joints, int M, int J, int loss_type, double push_factor,
                        double pull_factor, float* heat_loss, float* push_out, float* pull_out, hipStream_t s);
// lp_pose_loss_grad.  Every element of grad [N,C,R,R]: planes c < JH take g_heat[n] * heat_factor * 2 (p - g) m / (J R R),
// the others zeros (JH = 0: no heatmap plane; pred / gt / mask / g_heat are then not read)
void launch_heat_grad(const float* pred, const float* gt, const float* mask, const float* g_heat, int N, int C, int JH, int J,
                      int R, int S, double heat_factor, float* grad, hipStream_t s);
// after launch_heat_grad on the same stream: the cells of the tag channels that a counting slot names.  g_push / g_pull may
// be null, not both.  M * J <= 64 * 32: checked by the caller
void launch_tag_grad(const float* out, int N, int C, int R, int tag_offset, const int* joints, int M, int J, int loss_type,
                     double push_factor, double pull_factor, const float* g_push, const float* g_pull, float* grad,
                     hipStream_t s);

// ---- training-mode layers (layer_kernels.hip; lp_bn_* / lp_pw_* / lp_dw_*, layer_api.cpp) ------
// y = act(gamma * (x - mean) * invstd + beta) (+ res), out of place.  training: after launch_bn_stats(x, part) on the same
// stream; writes stat = [mean | invstd] x C (fp64) and moves running = [mean | var] x C.  !training: the running pair is the
// statistics; part and stat are not touched
void launch_bn_fwd(const float* x, const float* res, const double* part, const float* gamma, const float* beta,
                   float* running, float* y, double* stat, int N, int C, int HW, int act, bool training, double momentum,
                   double eps, hipStream_t s);
// two launches: the per-workgroup (sum g, sum g * xhat) partials -> part (bn_partial_doubles), then dx, dgamma, dbeta
void launch_bn_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const double* stat, double* part,
                   float* dx, float* dgamma, float* dbeta, int N, int C, int HW, int act, hipStream_t s);
// synchronised BatchNorm (lp_bn_sync_*): a rank's partials -> one fp64 row, the ranks' rows [W][.] in rank order -> the layer.
// part [C][S] pairs (S = bn_cut(N, C, HW).S) -> row = firsts[C] | seconds[C] (| cnt | 0 with tail), index order
void launch_bn_row(const double* part, int S, int C, double cnt, bool tail, double* row, hipStream_t s);
// rows [W][2C + 2] = sum | sumsq | count | 0; writes y, stat = mean[C] | invstd[C] | total count | 0, moves running
void launch_bn_sync_fwd(const float* x, const float* res, const double* rows, int W, const float* gamma, const float* beta,
                        float* running, float* y, double* stat, int N, int C, int HW, int act, double momentum, double eps,
                        hipStream_t s);
// bn_bwd_stats_kernel on the global pair of stat -> part (bn_partial_doubles) -> row [2C] = sum g | sum g * xhat
void launch_bn_sync_bwd_stats(const float* dy, const float* x, const float* gamma, const float* beta, const double* stat,
                              double* part, double* row, int N, int C, int HW, int act, hipStream_t s);
// rows [W][2C]; dx from the rank-order sums over n = stat[2C], dgamma / dbeta from rows[rank]
void launch_bn_sync_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const double* stat,
                        const double* rows, int W, int rank, float* dx, float* dgamma, float* dbeta, int N, int C, int HW,
                        int act, hipStream_t s);
// w [Cout][Cin] (transpose: its transpose) -> launch_pw's A fragments [ceil(M/32)][(K+1)/2][64] and ceil(M/32) * 32 zeros
void launch_pw_pack(const float* w, int Cout, int Cin, bool transpose, float* wp, float* zb, hipStream_t s);
// w [C][K*K] -> launch_dw's wdup [C][K*K][2] and C zeros
void launch_dw_pack(const float* w, int C, int K, float* wdup, float* zb, hipStream_t s);
// dw [Cout][Cin] = sum over n, p of dy[n][co][p] * x[n][ci][p]; part: pw_wgrad_slices(N * HW) * Cout * Cin floats
int pw_wgrad_slices(long NP);
void launch_pw_wgrad(const float* dy, const float* x, float* part, float* dw, int N, int HW, int Cout, int Cin,
                     hipStream_t s);
// depthwise K 3/5/7, stride S 1/2 (S = 2: even H, W): dx [N,C,H,W] and / or dw [C][K*K] (either may be null); part:
// dw_wgrad_slices(N, OH, OW) * C * K * K floats, needed for dw only
int dw_wgrad_slices(int N, int OH, int OW);
void launch_dw_backward(const float* dy, const float* x, const float* w, float* dx, float* part, float* dw, int N, int C,
                        int H, int W, int K, int S, hipStream_t s);

// out[i] = sum over s < S of part[s * stride + i] for i < count: fp64, index order, one rounding (slice_sum_kernel)
void launch_slice_sum(const float* part, int S, int stride, int count, float* out, hipStream_t s);

// ---- backward of the stem convolution and of the ConvTranspose2d(k4,s2,p1) pair (conv_grad_kernels.hip) ----
// wa [Ca][Cout][16] | wb [Cb][Cout][16] (wb null with Cb = 0) -> wp [Ca+Cb][Cout][16], what launch_deconv_raw and the data
// gradient read
void launch_deconv_pack(const float* wa, const float* wb, float* wp, int Ca, int Cb, int Cout, hipStream_t s);
// gxa / gxb [N,Ca|Cb,h,w] (both or neither; gxb null with Cb = 0; needs wp) and / or gwa / gwb [Ca|Cb][Cout][16] (likewise;
// needs xa / xb and part: deconv_wgrad_slices(N, h, w) * (Ca + Cb) * Cout * 16 floats); dy [N,Cout,2h,2w]
int deconv_wgrad_slices(int N, int h, int w);
void launch_deconv_backward(const float* dy, const float* xa, const float* xb, const float* wp, float* gxa, float* gxb,
                            float* part, float* gwa, float* gwb, int N, int Ca, int Cb, int Cout, int h, int w,
                            hipStream_t s);
// dw [32][27] of the stem from dy [N,32,H/2,W/2] and x [N,3,H,W] (even H, W); part: stem_wgrad_slices(N, H, W) * 864 floats
int stem_wgrad_slices(int N, int H, int W);
void launch_stem_wgrad(const float* dy, const float* x, float* part, float* dw, int N, int H, int W, hipStream_t s);

// ---- the dense K x K convolution as a training layer (dense_grad_kernels.hip; lp_conv_*, layer_api.cpp) ----
// plain weights -> launch_convk3's A fragments ws (convk_pack_bytes(M, Kt, K) bytes) and bout: ceil(M / 32) * 32 floats = bias
// (may be null: zeros).  !transpose: wa [Cout][Ca][K][K] | wb [Cout][Cb][K][K] (wb null with Cb = 0), M = Cout rows, Kt =
// Ca + Cb.  transpose: the data gradient's weights of ONE source wa [Cout][Ca][K][K]: M = Ca rows, Kt = Cout, taps flipped
size_t convk_pack_bytes(int M, int Kt, int K);
void launch_convk_pack(const float* wa, int Ca, const float* wb, int Cb, int Cout, int K, bool transpose, const float* bias,
                       void* ws, float* bout, hipStream_t s);
// z [planes][2 OH][2 OW] = dy [planes][OH][OW] at the even cells, zeros elsewhere (the stride-2 data gradient's operand)
void launch_dilate2(const float* dy, float* z, long planes, int OH, int OW, hipStream_t s);
// gx [planes][H][W] = the 2x2 cell sums of g [planes][2H][2W], one fixed order (the gradient of a nearest x2 upsample)
void launch_pool2(const float* g, float* gx, long planes, int H, int W, hipStream_t s);
// gwa [Cout][Ca][K][K] (and gwb, null with Cb = 0) from dy [N,Cout,OH,OW] and the sources [N,Ca|Cb,H,W] (read through a nearest
// x2 upsample when ups); part: conv_wgrad_slices(N, OH, OW) * Cout * (Ca + Cb) * K * K floats
int conv_wgrad_slices(int N, int OH, int OW);
void launch_conv_wgrad(const float* dy, const float* xa, const float* xb, float* part, float* gwa, float* gwb, int N, int Ca,
                       int Cb, int Cout, int H, int W, int K, int S, int ups, hipStream_t s);
// gbias [Cout] = per-channel sum of dy [N,Cout,HW]; part: Cout * conv_bias_slices(N, HW) doubles
int conv_bias_slices(int N, int HW);
void launch_conv_bias_grad(const float* dy, double* part, float* gbias, int N, int Cout, int HW, hipStream_t s);

}  // namespace lp
