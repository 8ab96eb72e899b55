// Host engine behind include/litepose_amd.h: reference state_dict ingestion, upload of the plan that plan.cpp builds
// (architecture bookkeeping, BatchNorm folding, weight packing, op and buffer lists), workspace planning and the launch
// sequence of one LitePose forward.  No torch, no Python: plain C++ + HIP runtime.
//
// Reference code this replaces (nothing is copied; semantics only):
//   lib/models/pose_mobilenet.py:137-156  forward (launch order below)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/litepose_amd.h"
#include "kernels.h"
#include "plan.h"

using namespace lp_plan;   // Tensor, Op / BOp, OpType, BufferPlan, Net: the host-only half (plan.cpp)

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_OK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(LP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

static_assert(ACT_NONE == lp::ACT_NONE && ACT_RELU == lp::ACT_RELU && ACT_RELU6 == lp::ACT_RELU6, "plan.h restates lp::Act");

const char* storage_name(const Net* n) { return n->storage == LP_STORAGE_F16 ? "f16" : "bf16"; }

}  // namespace

struct lp_net : lp_plan::Net {           // arch, tensors, storage and the plan: plan.h
    bool finalized = false;
    float* d_weights = nullptr;
    // last forward (for taps)
    std::vector<float*> last_ptr;
    int lastN = 0, lastH = 0, lastW = 0;
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> events;
    struct ProfEntry { std::string name, kernel; int64_t bytes, flops; int ev0, ev1; int64_t flops_valu; lp::LaunchNote launch; };   // flops_valu: the
    // depthwise / stem-conv share of `flops` (fp32 FMAs on the vector pipe); the rest are 1x1 / deconv FLOPs (matrix cores)
    std::vector<ProfEntry> prof_entries;   // one per LAUNCH of the last profiled forward
    int prof_ev = 0;                       // next free event
    // two internal streams: the plain and the mirrored half of a TTA batch are independent, so
    // their launch sequences are interleaved to overlap each other's kernel tails / launch gaps
    static constexpr int MAX_SIDE = 8;
    hipStream_t side[MAX_SIDE] = {};
    hipEvent_t ev_fork = nullptr, ev_join[MAX_SIDE] = {};
    int nstreams = 0;                      // 0 = default fan-out of 2 (lp_net_set_streams; no environment hook in csrc)
    // kernel-family switches (lp_net_set_option; the parity tests compare the forms)
    int opt_mb16 = 1;                      // 16x16-plane blocks: mb16_kernel (0: pw3 / dw_pair16 / pw3)
    int opt_mb16_run = 1;                  // ... a run of same-shape residual blocks per launch (0: one block)
    int opt_mb16_min = 48;                 // ... only for launches of at least this many images (one workgroup per image:
                                           //     a small batch leaves the chip empty; below it the pw3 / dw_pair16 / pw3 chain)
    int opt_mbt = 1, opt_mbt_s2 = 1;       // tiled fused blocks (mbtile_kernels.hip: launch_mbt)
    int opt_mbconv2 = 1;                   // 16-filter blocks in mbconv2_kernel (0: the unfused chain)
    int opt_mbtb = 1, opt_mbtb_s2 = 1;     // bf16 storage: whole-block kernels
    int opt_pw3d = 1;                      // fp32: small launches of the bf16x3 1x1 take the deep-prefetch form (0 off, 2 always)
    int opt_mbtd = 1;                      // bf16: the small residual blocks as bf16-E / dot2 workgroups, two per CU (0 off)
    int opt_mbtq = 1;                      // ... the small residual blocks as 4-wave workgroups, two per CU (0 off, 2 always)
    int opt_headb = 1;                     // bf16 storage: an output head (dw5 + dw5 + 1x1; plain head: dw5 + 1x1) in one launch
    int opt_headfuse = 1;                  // fp32: an output head in one launch, headfuse_kernel (0: the unfused chain)
    int opt_dwt = 2;                       // bf16 storage: matrix-core depthwise (0 never, 1 7x7, 2 + the heads' 5x5)
    int opt_stem = 1;                      // one-launch stem, stem4_kernel (0: stem_kernel + dwpw_kernel<3>)
    int opt_diag_dwpw = 0;                 // diagnostics of DESIGN 5b (tools/flake_hunt.py --diag), never production
    struct OptEntryT { const char* key; int lo, hi; int lp_net::*field; };
    static const std::vector<OptEntryT>& options();
    std::vector<char*> last_ptr_b;
    std::vector<char> last_stored_b;       // per buffer: written by the last forward (a fused block stores only its output)
    // BatchNorm re-calibration (lp_calib_*): a shadow net of the same arch whose plan folds the identity instead of the
    // BatchNorm (raw conv weights for the unfused launches), and the [gamma | beta | mean | var] rows of every BatchNorm
    struct CalibLayer { std::string bn; int C, div; size_t off; };
    struct Calib {
        lp_net* raw = nullptr;
        std::vector<CalibLayer> layers;    // launch order
        std::map<std::string, int> index;
        std::vector<float> h_bn;
        float* d_bn = nullptr;
        double momentum = 0.1;
        int64_t steps = 0;
        bool uploaded = false;
    };
    Calib* calib = nullptr;
};

namespace {

size_t buf_elems(const lp_net* n, int b, int N, int H, int W) {
    const int d = n->bufs.div[b];
    const size_t f = (size_t)N * n->bufs.ch[b] * (H / d) * (W / d);
    return (f + 127) / 128 * 128;
}

size_t buf_floats(const lp_net* n, int b, int N, int H, int W) {
    const int d = n->bufs.div[b];
    size_t f = (size_t)N * n->bufs.ch[b] * (H / d) * (W / d);
    return (f + 63) / 64 * 64;
}

// a buffer's share of the workspace: 16-bit elements under 16-bit storage
size_t buf_bytes(const lp_net* n, int b, int N, int H, int W) {
    return n->storage != LP_STORAGE_F32 ? buf_elems(n, b, N, H, W) * sizeof(uint16_t) : buf_floats(n, b, N, H, W) * sizeof(float);
}

// Every plane of a forward is H / div x W / div of its buffer (buf_floats, rounded down), while a strided kernel derives
// its output plane from its input plane (rounded up): the two agree only when the deepest divisor of THIS net divides H
// and W.  The divisors are 2 x a product of strides 1 / 2, so each divides the deepest one.
int size_multiple(const lp_net* n) {
    int m = 16;
    for (int d : n->bufs.div) m = std::max(m, d);
    return m;
}

int check_size(const lp_net* n, int H, int W) {
    const int m = size_multiple(n);
    if (H < m || W < m || (H % m) || (W % m))
        return fail(LP_ERR_INVALID_ARG, "H and W must be positive multiples of " + std::to_string(m) +
                                            " (the deepest plane of this net is 1/" + std::to_string(m) + " of the input)");
    return LP_OK;
}

}  // namespace

extern "C" {

const char* lp_last_error(void) { return g_err.c_str(); }
void lp_set_error_(const char* msg) { g_err = msg ? msg : ""; }
const char* lp_version(void) { return "litepose_amd 0.1 (gfx950, fp32 planar)"; }

int lp_net_create(lp_net** out, const lp_arch* a) {
    if (!out || !a) return fail(LP_ERR_INVALID_ARG, "null argument");
    lp_net* n = new lp_net();
    if (const int rc = init_arch(*n, *a)) {
        delete n;
        return fail(rc, lp_plan::last_error());
    }
    *out = n;
    return LP_OK;
}

static void calib_release(lp_net* n) {
    if (!n->calib) return;
    if (n->calib->d_bn) (void)hipFree(n->calib->d_bn);
    lp_net_destroy(n->calib->raw);
    delete n->calib;
    n->calib = nullptr;
}

void lp_net_destroy(lp_net* n) {
    if (!n) return;
    calib_release(n);
    if (n->d_weights) (void)hipFree(n->d_weights);
    for (auto e : n->events) (void)hipEventDestroy(e);
    for (int k = 0; k < lp_net::MAX_SIDE; ++k) {
        if (n->side[k]) (void)hipStreamDestroy(n->side[k]);
        if (n->ev_join[k]) (void)hipEventDestroy(n->ev_join[k]);
    }
    if (n->ev_fork) (void)hipEventDestroy(n->ev_fork);
    delete n;
}

int lp_net_num_keys(const lp_net* n) { return n ? (int)n->tensors.size() : 0; }

const char* lp_net_key(const lp_net* n, int i, int64_t shape_out[4], int* ndim_out) {
    if (!n || i < 0 || i >= (int)n->tensors.size()) return nullptr;
    const Tensor& t = n->tensors[i];
    if (shape_out)
        for (size_t d = 0; d < 4; ++d) shape_out[d] = d < t.shape.size() ? t.shape[d] : 1;
    if (ndim_out) *ndim_out = (int)t.shape.size();
    return t.key.c_str();
}

int lp_net_set_weight(lp_net* n, const char* key, const float* h, const int64_t* shape, int ndim) {
    if (!n || !key) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (n->calib) return fail(LP_ERR_INVALID_ARG, "a calibration is open on this handle: lp_calib_end() first");
    std::string k(key);
    // checkpoints saved from DataParallel / DDP carry a "module." prefix
    if (k.rfind("module.", 0) == 0) k = k.substr(7);
    auto it = n->index.find(k);
    if (it == n->index.end()) return fail(LP_ERR_UNKNOWN_KEY, "unexpected key in state_dict: " + k);
    Tensor& t = n->tensors[it->second];
    if (t.is_counter) { t.is_set = true; return LP_OK; }
    if (!h) return fail(LP_ERR_INVALID_ARG, "null data for " + k);
    if (ndim != (int)t.shape.size()) return fail(LP_ERR_SHAPE, "rank mismatch for " + k);
    for (int d = 0; d < ndim; ++d)
        if (shape[d] != t.shape[d]) return fail(LP_ERR_SHAPE, "size mismatch for " + k);
    t.data.assign(h, h + t.numel());
    t.is_set = true;
    n->finalized = false;
    return LP_OK;
}

int lp_net_get_weight(const lp_net* n, const char* key, float* h, int64_t numel) {
    if (!n || !key || !h) return fail(LP_ERR_INVALID_ARG, "null argument");
    auto it = n->index.find(key);
    if (it == n->index.end()) return fail(LP_ERR_UNKNOWN_KEY, std::string("unknown key ") + key);
    const Tensor& t = n->tensors[it->second];
    if (t.is_counter || !t.is_set || numel != t.numel()) return fail(LP_ERR_SHAPE, "numel mismatch / unset");
    std::memcpy(h, t.data.data(), sizeof(float) * (size_t)numel);
    return LP_OK;
}

int lp_net_finalize(lp_net* n, int strict) {
    if (!n) return fail(LP_ERR_INVALID_ARG, "null net");
    for (auto& t : n->tensors) {
        if (t.is_counter) continue;
        if (!t.is_set) {
            if (strict) return fail(LP_ERR_MISSING_WEIGHT, "missing key in state_dict: " + t.key);
            // non-strict: BN identity / zero conv, like a freshly constructed module would not be;
            // we require weights, so default to identity BN and zero weights.
            t.data.assign((size_t)t.numel(), 0.f);
            const bool bn_scale = t.key.size() > 7 && t.shape.size() == 1 &&
                                  (t.key.rfind(".weight") == t.key.size() - 7 ||
                                   t.key.rfind("running_var") != std::string::npos);
            if (bn_scale && !(n->arch.family == 1 && t.key.rfind("final_", 0) == 0)) t.data.assign((size_t)t.numel(), 1.f);
        }
    }
    if (n->arch.family == 1 && n->storage != LP_STORAGE_F32)
        return fail(LP_ERR_UNSUPPORTED, "pose_resnet family: fp32 storage only (no 16-bit dense-conv kernels yet)");
    if (const int rc = build(*n)) return fail(rc, lp_plan::last_error());
    if (n->d_weights) { (void)hipFree(n->d_weights); n->d_weights = nullptr; }
    HIP_OK(hipMalloc((void**)&n->d_weights, n->h_packed.size() * sizeof(float)));
    HIP_OK(hipMemcpy(n->d_weights, n->h_packed.data(), n->h_packed.size() * sizeof(float),
                     hipMemcpyHostToDevice));
    n->finalized = true;
    return LP_OK;
}

size_t lp_net_workspace_bytes(const lp_net* n, int N, int H, int W) {
    if (!n || !n->finalized) return 0;
    if (N < 1 || check_size(n, H, W) != LP_OK) return 0;      // lp_last_error names the multiple
    // Buffers are planned one-per-tensor (no aliasing): 288 GB of HBM make the ~6x
    // over-allocation irrelevant and every block-boundary tensor stays tappable.
    size_t bytes = 256;
    for (size_t b = 0; b < n->bufs.ch.size(); ++b) bytes += buf_bytes(n, (int)b, N, H, W);
    return bytes;
}

static constexpr bool deconv4_enabled() { return true; }

int lp_net_profile_launches(const lp_net* n, int32_t* grid_wgs, int32_t* wg_threads, int32_t* lds_bytes,
                            int32_t* wgs_per_cu, int cap) {
    if (!n || !n->profiling || n->prof_entries.empty())
        return fail(LP_ERR_INVALID_ARG, "profiling not enabled / no forward yet");
    const int cnt = std::min((int)n->prof_entries.size(), cap);
    for (int i = 0; i < cnt; ++i) {
        const auto& l = n->prof_entries[i].launch;
        if (grid_wgs) grid_wgs[i] = l.grid;
        if (wg_threads) wg_threads[i] = l.block;
        if (lds_bytes) lds_bytes[i] = l.lds;
        if (wgs_per_cu) wgs_per_cu[i] = l.wgs_per_cu;
    }
    return cnt;
}

}  // extern "C"

namespace {

// ---- what lp_net_forward and forward_bf16 share: workspace layout, profiling events, the K-stream fan-out ----

// one block of the workspace per buffer, in id order; the two outputs are the caller's fp32 tensors.  esz: bytes per element
void layout_buffers(const lp_net* n, void* ws, int NB, int H, int W, float* d_out0, float* d_out1, std::vector<char*>& ptr,
                    std::vector<int>& esz) {
    const size_t nbuf = n->bufs.ch.size();
    ptr.resize(nbuf);
    esz.assign(nbuf, n->storage != LP_STORAGE_F32 ? 2 : 4);
    char* p = (char*)ws;
    for (size_t b = 0; b < nbuf; ++b) {
        ptr[b] = p;
        p += buf_bytes(n, (int)b, NB, H, W);
    }
    ptr[n->out0_buf] = (char*)d_out0;
    ptr[n->out1_buf] = (char*)d_out1;
    esz[n->out0_buf] = esz[n->out1_buf] = 4;
}

// profiling: one entry per launch, bracketed by consecutive events on the launch stream
int prof_begin(lp_net* n, size_t nops, hipStream_t s) {
    lp::launch_notes = n->profiling;
    if (!n->profiling) return LP_OK;
    while (n->events.size() < 2 * nops + 2) {
        hipEvent_t e;
        HIP_OK(hipEventCreate(&e));
        n->events.push_back(e);
    }
    n->prof_entries.clear();
    n->prof_ev = 0;
    HIP_OK(hipEventRecord(n->events[0], s));
    return LP_OK;
}
int prof_mark(lp_net* n, hipStream_t s, const std::string& name, int64_t by, int64_t fl, int64_t fl_valu) {
    if (!n->profiling) return LP_OK;
    hipError_t e = hipEventRecord(n->events[n->prof_ev + 1], s);
    if (e != hipSuccess) return fail(LP_ERR_HIP, hipGetErrorString(e));
    n->prof_entries.push_back({name, lp::last_kernel_tag, by, fl, n->prof_ev, n->prof_ev + 1, fl_valu, lp::last_launch});
    ++n->prof_ev;
    return LP_OK;
}

// K internal streams: the batch (and its mirrored copy) is cut into K independent parts whose launch sequences
// interleave, hiding kernel tails / launch gaps of the small late layers.  run(images, buffers, stream, input, flip_from,
// x_batch) launches one part
template <class Run>
int fan_out(lp_net* n, const float* d_x, int N, int H, int W, int flip, hipStream_t s, const std::vector<char*>& ptr,
            const std::vector<int>& esz, Run run) {
    const int NB = flip == 2 ? 2 * N : N;
    const int mode = n->nstreams > 0 ? n->nstreams : 2;     // default fan-out of 2 (lp_net_set_streams overrides)
    int K = mode > lp_net::MAX_SIDE ? lp_net::MAX_SIDE : mode;
    while (K > 1 && (n->profiling || NB % K != 0 || (flip == 2 && N % (NB / K) != 0))) K >>= 1;
    if (K <= 1) return run(NB, ptr, s, d_x, flip == 0 ? NB : (flip == 1 ? 0 : N), N);
    for (int k = 0; k < K; ++k)
        if (!n->side[k]) {
            HIP_OK(hipStreamCreateWithFlags(&n->side[k], hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&n->ev_join[k], hipEventDisableTiming));
        }
    if (!n->ev_fork) HIP_OK(hipEventCreateWithFlags(&n->ev_fork, hipEventDisableTiming));
    const int np = NB / K;
    HIP_OK(hipEventRecord(n->ev_fork, s));
    for (int k = 0; k < K; ++k) {
        const int g0 = k * np;                                   // first image of this part
        std::vector<char*> ph(ptr.size());
        for (size_t b = 0; b < ptr.size(); ++b) {
            const int d = n->bufs.div[b];
            ph[b] = ptr[b] + (size_t)g0 * n->bufs.ch[b] * (H / d) * (W / d) * esz[b];
        }
        const bool mirrored = flip == 1 || (flip == 2 && g0 >= N);
        const float* xs = d_x + (size_t)(g0 % N) * 3 * H * W;
        HIP_OK(hipStreamWaitEvent(n->side[k], n->ev_fork, 0));
        const int rc = run(np, ph, n->side[k], xs, mirrored ? 0 : np, np);
        if (rc) return rc;
        HIP_OK(hipEventRecord(n->ev_join[k], n->side[k]));
    }
    for (int k = 0; k < K; ++k) HIP_OK(hipStreamWaitEvent(s, n->ev_join[k], 0));
    return LP_OK;
}

// lp_net_forward for LP_STORAGE_BF16 / LP_STORAGE_F16: same launch order, stream fan-out and profiling contract as the fp32 path
int forward_bf16(lp_net* n, const float* d_x, int N, int H, int W, int flip, float* d_out0, float* d_out1, void* ws,
                 size_t ws_bytes, hipStream_t s) {
    const int NB = flip == 2 ? 2 * N : N;
    if (ws_bytes < lp_net_workspace_bytes(n, NB, H, W) || ((uintptr_t)ws & 255))
        return fail(LP_ERR_WORKSPACE, "workspace too small or not 256-byte aligned");
    const bool f16 = n->storage == LP_STORAGE_F16;      // every launch below takes the format last
    std::vector<char*> ptr;
    std::vector<int> esz;
    layout_buffers(n, ws, NB, H, W, d_out0, d_out1, ptr, esz);
    const float* Wt = n->d_weights;
    if (const int rc = prof_begin(n, n->bops.size(), s)) return rc;
    std::vector<char> stored(ptr.size(), 0);
    auto run = [&](int NBp, const std::vector<char*>& ptr, hipStream_t s, const float* xsrc, int flip_from,
                   int x_batch) -> int {
        auto mark = [&](const std::string& name, int64_t by, int64_t fl, int64_t fl_valu) {
            return prof_mark(n, s, name, by, fl, fl_valu);
        };
        for (size_t bi = 0; bi < n->bops.size(); ++bi) {
            const BOp& o = n->bops[bi];
            const int ih = H / o.in_div, iw = W / o.in_div, oh = H / o.out_div, ow = W / o.out_div;
            int64_t by = 0, fl = 0;
            bool ok = true;
            // the whole 7x7 block in one launch (mbtb_kernel / mbtb_s2_kernel, round 3): expand / depthwise / project,
            // the two expanded tensors never stored.  Option "mbtb" = 0 keeps the chain below
            if (o.type == OP_PW && o.inB < 0 && !o.out_f32 && o.act == lp::ACT_RELU6 && bi + 2 < n->bops.size()) {
                const BOp& dw = n->bops[bi + 1];
                const BOp& pw = n->bops[bi + 2];
                if (dw.type == OP_DW && dw.inA == o.out && dw.K == 7 && (dw.S == 1 || dw.S == 2) && dw.wrow_off &&
                    dw.act == lp::ACT_RELU6 && pw.type == OP_PW && pw.inA == dw.out && pw.inB < 0 && !pw.out_f32 &&
                    pw.act == lp::ACT_NONE && (pw.res < 0 || pw.res == o.inA) &&
                    lp::launch_mbtb(ptr[o.inA], Wt + o.w_off, Wt + o.b_off, Wt + dw.wrow_off, Wt + pw.w_off,
                                    Wt + pw.b_off, pw.res >= 0 ? ptr[pw.res] : nullptr, ptr[pw.out], NBp, o.Ca, o.Cout,
                                    pw.Cout, ih, iw, dw.K, dw.S, s, n->opt_mbtb, n->opt_mbtb_s2, n->opt_mbtq,
                                    dw.wrow2_off ? Wt + dw.wrow2_off : nullptr, n->opt_mbtd, f16)) {
                    const int64_t ipx = (int64_t)ih * iw, opx = ipx / (dw.S * dw.S);
                    if (const int rc = mark(o.name + "+dw+point_conv",     // short: lp_net_profile names are 47 chars
                                            2ll * NBp * (ipx * o.Ca + opx * pw.Cout * (pw.res >= 0 ? 2ll : 1ll)),
                                            2ll * NBp * (ipx * o.Ca * o.Cout + opx * ((int64_t)o.Cout * 49 + (int64_t)o.Cout * pw.Cout)),
                                            2ll * NBp * opx * (int64_t)o.Cout * 49))
                        return rc;
                    stored[pw.out] = 1;
                    bi += 2;                                    // the depthwise and the project ran inside the launch
                    continue;
                }
            }
            // the whole stem in one launch (stem4_kernel<C0, true>, round 6; option "stem" = 0: the three launches below, what
            // the per-launch parity tests run)
            if (o.type == OP_STEM && n->opt_stem && o.st_w0 && bi + 2 < n->bops.size()) {
                const BOp& dw = n->bops[bi + 1];
                const BOp& pw = n->bops[bi + 2];
                if (dw.type == OP_DW && dw.K == 3 && dw.S == 1 && pw.type == OP_PW && pw.inA == dw.out && !pw.out_f32 &&
                    lp::launch_stem3b(xsrc, Wt + o.st_w0, Wt + o.b_off, Wt + o.st_w1, Wt + o.st_b1, Wt + o.st_w2,
                                      Wt + o.st_b2, ptr[pw.out], NBp, H, W, pw.Cout, flip_from, x_batch, s, f16)) {
                    const int64_t opx = (int64_t)oh * ow;
                    if (const int rc = mark("stem.conv3x3s2+dw3+pw",
                                            (int64_t)NBp * (12ll * H * W + 64ll * opx) + (int64_t)NBp * 2 * 64ll * opx +
                                                (int64_t)NBp * (64ll + 2ll * pw.Cout) * opx,
                                            2ll * NBp * opx * (32ll * 27 + 32ll * 9 + 32ll * pw.Cout),
                                            2ll * NBp * opx * (32ll * 27 + 32ll * 9)))
                        return rc;
                    stored[pw.out] = 1;
                    bi += 2;
                    continue;
                }
            }
            // an output head in one launch (headb_kernel, round 6: both 5x5 depthwise convs + the dual-source 1x1; option
            // "headb" = 0: the three launches below, what the per-launch parity tests run).  Needs the matrix-core depthwise
            // (option "dwt" >= 2): its results are the SAME bits as dwt_kernel<5>'s
            if (o.type == OP_DW && o.K == 5 && o.S == 1 && n->opt_headb && n->opt_dwt >= 2 && o.wt_off &&
                bi + 2 < n->bops.size()) {
                const BOp& d2 = n->bops[bi + 1];
                const BOp& pw = n->bops[bi + 2];
                if (d2.type == OP_DW && d2.K == 5 && d2.S == 1 && d2.wt_off && o.act == lp::ACT_RELU &&
                    d2.act == lp::ACT_RELU && pw.type == OP_PW && pw.out_f32 && pw.inA == o.out && pw.inB == d2.out &&
                    pw.act == lp::ACT_NONE && pw.res < 0 &&
                    lp::launch_headb(ptr[o.inA], o.Ca, ptr[d2.inA], d2.Ca, Wt + o.wt_off, Wt + o.w_off, Wt + d2.wt_off,
                                     Wt + d2.w_off, Wt + pw.w_off, reinterpret_cast<float*>(ptr[pw.out]), NBp, ih, iw, o.K,
                                     pw.Cout, s, f16)) {
                    const int64_t px = (int64_t)NBp * oh * ow, C = o.Ca + d2.Ca;
                    if (const int rc = mark("final." + pw.name.substr(6, pw.name.find('.', 6) - 6) + ".dw5+dw5+pw",
                                            2ll * px * 2 * C + px * (2ll * C + 4ll * pw.Cout),
                                            2ll * px * (C * 25 + C * (int64_t)pw.Cout), 2ll * px * C * 25))
                        return rc;
                    stored[pw.out] = 1;
                    bi += 2;
                    continue;
                }
            }
            // the one-source head of a plain_head net (dw5 + the 1x1) in one launch: headb_kernel's one-source form, the SAME bits
            // as dwt_kernel<5> + pwb_kernel
            if (o.type == OP_DW && o.K == 5 && o.S == 1 && n->opt_headb && n->opt_dwt >= 2 && o.wt_off && o.act == lp::ACT_RELU &&
                bi + 1 < n->bops.size()) {
                const BOp& pw = n->bops[bi + 1];
                if (pw.type == OP_PW && pw.out_f32 && pw.inA == o.out && pw.inB < 0 && pw.act == lp::ACT_NONE && pw.res < 0 &&
                    lp::launch_headb(ptr[o.inA], o.Ca, nullptr, 0, Wt + o.wt_off, Wt + o.w_off, nullptr, nullptr,
                                     Wt + pw.w_off, reinterpret_cast<float*>(ptr[pw.out]), NBp, ih, iw, o.K, pw.Cout, s, f16)) {
                    const int64_t px = (int64_t)NBp * oh * ow, C = o.Ca;
                    if (const int rc = mark("final." + pw.name.substr(6, pw.name.find('.', 6) - 6) + ".dw5+pw",
                                            2ll * px * 2 * C + px * (2ll * C + 4ll * pw.Cout),
                                            2ll * px * (C * 25 + C * (int64_t)pw.Cout), 2ll * px * C * 25))
                        return rc;
                    stored[pw.out] = 1;
                    ++bi;
                    continue;
                }
            }
            switch (o.type) {
                case OP_STEM:
                    lp::launch_stemb(xsrc, Wt + o.w_off, Wt + o.b_off, ptr[o.out], NBp, H, W, flip_from, x_batch, s, f16);
                    by = (int64_t)NBp * (12ll * H * W + 64ll * oh * ow);
                    fl = 2ll * NBp * 32 * 27 * oh * ow;
                    break;
                case OP_DW:
                    {
                        // the stride-1 7x7 / 5x5 depthwise runs as banded matrix products on the matrix cores
                        // (dwt_kernel) wherever its shape rule admits the plane: default since round 3 (S@448 b32:
                        // 5.60 -> 4.82 ms/step, every launch within 1 bf16 ulp of the emulation like dwb_kernel).
                        // Option "dwt" (the tests compare the forms in one process): 0 = dwb_kernel everywhere,
                        // 1 = 7x7 only, 2 (default) = 7x7 and the heads' 5x5
                        const int dwt = n->opt_dwt;
                        ok = dwt && o.wt_off && o.S == 1 && (o.K == 7 || (o.K == 5 && dwt >= 2)) &&
                             lp::launch_dwt(ptr[o.inA], Wt + o.wt_off, Wt + o.w_off, ptr[o.out], NBp, o.Ca, ih, iw,
                                            o.K, o.act, s, f16);
                        if (!ok)
                            ok = lp::launch_dwb(ptr[o.inA], Wt + o.w_off, ptr[o.out], NBp, o.Ca, ih, iw, o.K, o.S,
                                                o.act, s, f16);
                    }
                    by = 2ll * NBp * o.Ca * ((int64_t)ih * iw + (int64_t)oh * ow);
                    fl = 2ll * NBp * o.Ca * o.K * o.K * oh * ow;
                    break;
                case OP_PW:
                    ok = lp::launch_pwb(ptr[o.inA], o.Ca, o.inB >= 0 ? ptr[o.inB] : nullptr, o.Cb, Wt + o.w_off,
                                        Wt + o.b_off, o.res >= 0 ? ptr[o.res] : nullptr, ptr[o.out], NBp, oh * ow,
                                        o.Cout, o.act, o.out_f32, s, f16);
                    by = (int64_t)NBp * oh * ow *
                         (2ll * (o.Ca + o.Cb) + (o.out_f32 ? 4ll : 2ll) * o.Cout + (o.res >= 0 ? 2ll * o.Cout : 0));
                    fl = 2ll * NBp * oh * ow * (int64_t)(o.Ca + o.Cb) * o.Cout;
                    break;
                case OP_DECONV:
                    ok = lp::launch_deconvb(ptr[o.inA], o.Ca, o.inB >= 0 ? ptr[o.inB] : nullptr, o.Cb, Wt + o.w_off, Wt + o.b_off, ptr[o.out],
                                            NBp, ih, iw, o.Cout, s, f16);
                    by = 2ll * NBp * ((int64_t)(o.Ca + o.Cb) * ih * iw + (int64_t)o.Cout * oh * ow);
                    fl = 2ll * NBp * (int64_t)(o.Ca + o.Cb) * o.Cout * 4 * oh * ow;
                    break;
                default:                     // OP_DWPW / OP_CONVK: not on a 16-bit plan
                    ok = false;
                    break;
            }
            if (!ok) return fail(LP_ERR_UNSUPPORTED, std::string(storage_name(n)) + " storage: unsupported layer shape at " + o.name);
            stored[o.out] = 1;
            if (const int rc = mark(o.name, by, fl, (o.type == OP_STEM || o.type == OP_DW) ? fl : 0)) return rc;
        }
        return LP_OK;
    };
    if (const int rc = fan_out(n, d_x, N, H, W, flip, s, ptr, esz, run)) return rc;
    HIP_OK(hipGetLastError());
    n->last_ptr_b = ptr;
    n->last_stored_b = stored;
    n->last_ptr.assign(1, nullptr);          // "a forward has run"
    n->lastN = NB;
    n->lastH = H;
    n->lastW = W;
    return LP_OK;
}

}  // namespace

extern "C" {

int lp_net_forward(lp_net* n, const float* d_x, int N, int H, int W, int flip, float* d_out0,
                   float* d_out1, void* ws, size_t ws_bytes, void* stream) {
    if (!n || !d_x || !d_out0 || !d_out1 || !ws) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (!n->finalized) return fail(LP_ERR_NOT_FINALIZED, "lp_net_finalize() has not been called");
    if (N < 1) return fail(LP_ERR_INVALID_ARG, "N must be positive");
    if (const int rc = check_size(n, H, W)) return rc;           // both storage paths: before any buffer is laid out
    if (flip < 0 || flip > 2) return fail(LP_ERR_INVALID_ARG, "flip must be 0, 1 or 2");
    // a stale error of this thread (e.g. a hipGraph capture that another thread's call invalidated) must not be
    // mistaken for a failure of the launches below
    (void)hipGetLastError();
    if (n->storage != LP_STORAGE_F32)
        return forward_bf16(n, d_x, N, H, W, flip, d_out0, d_out1, ws, ws_bytes, (hipStream_t)stream);
    const int NB = flip == 2 ? 2 * N : N;             // images through the network
    if (ws_bytes < lp_net_workspace_bytes(n, NB, H, W) || ((uintptr_t)ws & 255))
        return fail(LP_ERR_WORKSPACE, "workspace too small or not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    std::vector<char*> bptr;
    std::vector<int> esz;
    layout_buffers(n, ws, NB, H, W, d_out0, d_out1, bptr, esz);
    const float* Wt = n->d_weights;
    if (const int rc = prof_begin(n, n->ops.size(), s)) return rc;
    auto run = [&](int NB, const std::vector<char*>& bptr, hipStream_t s, const float* xsrc, int flip_from,
                   int x_batch) -> int {
    std::vector<float*> ptr(bptr.size());
    for (size_t b = 0; b < ptr.size(); ++b) ptr[b] = reinterpret_cast<float*>(bptr[b]);
    auto prof_mark = [&](const std::string& name, int64_t by, int64_t fl, int64_t fl_valu) -> int {
        return ::prof_mark(n, s, name, by, fl, fl_valu);
    };
    for (size_t i = 0; i < n->ops.size(); ++i) {
        const Op& o = n->ops[i];
        const int ih = H / o.in_div, iw = W / o.in_div, oh = H / o.out_div, ow = W / o.out_div;
        int64_t by = 0, fl = 0;
        if (o.type == OP_PW && o.fuse_next && i + 1 < n->ops.size() && n->ops[i + 1].type == OP_DWPW) {
            // whole InvBottleneck in one launch when the shape allows it
            const Op& d = n->ops[i + 1];
            // 16x16 planes (mb16_kernel): the whole RUN of same-shape residual blocks that follows in one launch --
            // a block's output is the next block's input in the kernel's own register layout (mb16_kernels.hip)
            if (n->opt_mb16 && NB >= n->opt_mb16_min && o.ws_off && d.ws_off && d.wrow_off &&
                lp::mb16_supported(o.Ca, o.Cout, d.Cout, ih, iw, d.K, d.S, d.res >= 0)) {
                auto bytes_of = [&](const Op& e, const Op& p) {
                    return 4ll * NB * oh * ow * (e.Ca + e.Cout) + 4ll * NB * oh * ow * (int64_t)p.Ca +
                           4ll * NB * oh * ow * (2ll * p.Ca + (int64_t)p.Cout * (p.res >= 0 ? 2 : 1));
                };
                auto flops_of = [&](const Op& e, const Op& p) {
                    return 2ll * NB * oh * ow * (int64_t)e.Ca * e.Cout +
                           2ll * NB * oh * ow * ((int64_t)p.Ca * p.K * p.K + (int64_t)p.Ca * p.Cout);
                };
                lp::Mb16Run r;
                memset(&r, 0, sizeof(r));
                size_t last = i;                                   // index of the run's last expand op
                int64_t rby = 0, rfl = 0, rdw = 0;
                for (size_t k = i; k + 1 < n->ops.size() && r.nblocks < lp::MB16_MAX_RUN; k += 2) {
                    const Op& e = n->ops[k];
                    const Op& p = n->ops[k + 1];
                    if (e.type != OP_PW || !e.fuse_next || p.type != OP_DWPW || !e.ws_off || !p.ws_off || !p.wrow_off) break;
                    if (k > i) {        // a follower: same shape, residual on its own input, fed by the previous block
                        if (d.res < 0 || p.res != e.inA || e.inA != n->ops[k - 1].out || e.Ca != o.Ca ||
                            e.Cout != o.Cout || p.Cout != d.Cout || p.K != d.K || p.S != d.S ||
                            e.in_div != o.in_div || p.out_div != d.out_div || !n->opt_mb16_run)
                            break;
                    } else if (d.res >= 0 && d.res != o.inA) break;
                    const int b = r.nblocks++;
                    r.w1s[b] = Wt + e.ws_off; r.b1f[b] = Wt + e.b_off; r.wrow[b] = Wt + p.wrow_off;
                    r.w2s[b] = Wt + p.ws_off; r.b2f[b] = Wt + p.b2_off; r.out[b] = ptr[p.out];
                    rby += bytes_of(e, p); rfl += flops_of(e, p);
                    rdw += 2ll * NB * oh * ow * (int64_t)p.Ca * p.K * p.K;
                    last = k;
                    if (d.res < 0) break;                          // a block that changes the channel count runs alone
                }
                if (r.nblocks >= 1 && lp::launch_mb16(ptr[o.inA], r, d.res >= 0, NB, o.Ca, o.Cout, d.Cout, ih, iw, d.K,
                                                      d.S, s)) {
                    const Op& pl = n->ops[last + 1];
                    std::string nm = o.name + "+" + d.name.substr(d.name.rfind('.', d.name.find('+')) + 1);
                    if (r.nblocks > 1) {                           // "stage.2.1-9.inv+depth_conv+point_conv"
                        const std::string pfx = o.name.substr(0, o.name.rfind('.'));          // stage.2.1
                        const std::string lpf = pl.name.substr(0, pl.name.rfind('.', pl.name.find('+')));
                        nm = pfx + "-" + lpf.substr(lpf.rfind('.') + 1) + nm.substr(pfx.size());
                    }
                    const int rc = prof_mark(nm, rby, rfl, rdw);
                    if (rc) return rc;
                    i = last + 1;
                    continue;
                }
            }
            if ((o.ws_off && d.ws_off && d.wrow_off &&
                 lp::launch_mbt(ptr[o.inA], Wt + o.ws_off, Wt + o.b_off, Wt + d.wrow_off, Wt + d.ws_off, Wt + d.b2_off,
                                d.res >= 0 ? ptr[d.res] : nullptr, ptr[d.out], NB, o.Ca, o.Cout, d.Cout, ih, iw, d.K,
                                d.S, s, n->opt_mbt, n->opt_mbt_s2)) ||
                lp::launch_mbconv(ptr[o.inA], Wt + o.w_off, Wt + o.b_off, Wt + d.w_off, Wt + d.b_off,
                                  Wt + d.w2_off, Wt + d.b2_off, d.res >= 0 ? ptr[d.res] : nullptr, ptr[d.out],
                                  NB, o.Ca, o.Cout, d.Cout, ih, iw, d.K, d.S, s,
                                  d.wpair_off ? Wt + d.wpair_off : nullptr, o.ws_off ? Wt + o.ws_off : nullptr,
                                  d.wrow_off ? Wt + d.wrow_off : nullptr, n->opt_mbconv2)) {
                // B_op accounting of the three reference ops this launch replaces (expand at the input
                // resolution; depthwise out / project at the block's output resolution)
                {
                    const int64_t doh = H / d.out_div, dow = W / d.out_div;
                    const int rc = prof_mark(
                        o.name + "+" + d.name.substr(d.name.rfind('.', d.name.find('+')) + 1),
                        4ll * NB * oh * ow * (o.Ca + o.Cout) + 4ll * NB * oh * ow * (int64_t)d.Ca +
                            4ll * NB * doh * dow * (2ll * d.Ca + (int64_t)d.Cout * (d.res >= 0 ? 2 : 1)),
                        2ll * NB * oh * ow * (int64_t)o.Ca * o.Cout +
                            2ll * NB * doh * dow * ((int64_t)d.Ca * d.K * d.K + (int64_t)d.Ca * d.Cout),
                        2ll * NB * doh * dow * (int64_t)d.Ca * d.K * d.K);
                    if (rc) return rc;
                }
                ++i;
                continue;
            }
        }
        if (n->opt_stem && o.type == OP_STEM && i + 2 < n->ops.size() && n->ops[i + 1].type == OP_DW &&
            n->ops[i + 2].type == OP_PW && o.st_w0) {
            const Op& dw = n->ops[i + 1];
            const Op& pw = n->ops[i + 2];
            if (lp::launch_stem3(xsrc, Wt + o.st_w0, Wt + o.b_off, Wt + o.st_w1, Wt + dw.b_off, Wt + o.st_w2,
                                 Wt + o.st_b2, ptr[pw.out], NB, H, W, pw.Cout, flip_from, x_batch, s)) {
                // B_op accounting of the three reference ops this launch replaces
                const int rc = prof_mark("stem.conv3x3s2+dw3+pw",
                                         4ll * NB * (3ll * H * W + 32ll * oh * ow) + 4ll * NB * 32 * 2ll * oh * ow +
                                             4ll * NB * oh * ow * (32 + pw.Cout),
                                         2ll * NB * oh * ow * (32ll * 27 + 32ll * 9 + 32ll * pw.Cout),
                                         2ll * NB * oh * ow * (32ll * 27 + 32ll * 9));
                if (rc) return rc;
                i += 2;
                continue;
            }
        }
        if (o.type == OP_DW && o.K == 3 && o.S == 1 && o.act == lp::ACT_RELU6 && i + 1 < n->ops.size() &&
            n->ops[i + 1].type == OP_PW && n->ops[i + 1].inA == o.out && n->ops[i + 1].inB < 0 && n->ops[i + 1].res < 0 &&
            n->ops[i + 1].act == lp::ACT_NONE && n->ops[i + 1].has_bias) {
            // stem: dw3 + 1x1 in one launch (dwpw_kernel<3>): the 32-channel dw3 output stays in LDS
            const Op& pw = n->ops[i + 1];
            if (lp::launch_dwpw(ptr[o.inA], Wt + o.w_off, Wt + o.b_off, Wt + pw.w_off, Wt + pw.b_off, nullptr,
                                      ptr[pw.out], NB, o.Ca, ih, iw, o.K, o.S, pw.Cout, s, n->opt_diag_dwpw)) {
                const int64_t px = (int64_t)NB * oh * ow;
                const int rc = prof_mark(o.name + "+pw", 4ll * px * (2ll * o.Ca) + 4ll * px * (o.Ca + pw.Cout),
                                         2ll * px * ((int64_t)o.Ca * o.K * o.K + (int64_t)o.Ca * pw.Cout),
                                         2ll * px * (int64_t)o.Ca * o.K * o.K);
                if (rc) return rc;
                ++i;
                continue;
            }
        }
        if (n->opt_headfuse && o.type == OP_DW && o.K == 5 && o.S == 1 && o.act == lp::ACT_RELU && i + 1 < n->ops.size() &&
            n->ops[i + 1].type == OP_PW && n->ops[i + 1].inA == o.out && n->ops[i + 1].inB < 0 && n->ops[i + 1].res < 0 &&
            n->ops[i + 1].act == lp::ACT_NONE && (n->ops[i + 1].out == n->out0_buf || n->ops[i + 1].out == n->out1_buf)) {
            // one-source output head (plain_head): the 5x5 depthwise and the 1x1 in one launch, bit-identical to dw + pw
            const Op& pw = n->ops[i + 1];
            if (lp::launch_headfuse(ptr[o.inA], o.Ca, nullptr, 0, o.wpair_off ? Wt + o.wpair_off : nullptr, nullptr,
                                    Wt + pw.w_off, ptr[pw.out], NB, oh, ow, o.K, pw.Cout, s)) {
                const int64_t px = (int64_t)NB * oh * ow;
                const int rc = prof_mark("final." + pw.name.substr(6, pw.name.find('.', 6) - 6) + ".dw5+pw",
                                         4ll * px * (2ll * o.Ca) + 4ll * px * (o.Ca + pw.Cout),
                                         2ll * px * ((int64_t)o.Ca * o.K * o.K + (int64_t)o.Ca * pw.Cout),
                                         2ll * px * (int64_t)o.Ca * o.K * o.K);
                if (rc) return rc;
                ++i;
                continue;
            }
        }
        if (n->opt_headfuse && o.type == OP_DW && i + 2 < n->ops.size() && n->ops[i + 1].type == OP_DW && n->ops[i + 2].type == OP_PW &&
            n->ops[i + 2].inA == o.out && n->ops[i + 2].inB == n->ops[i + 1].out && o.S == 1 && n->ops[i + 1].S == 1 &&
            o.K == n->ops[i + 1].K && o.act == lp::ACT_RELU && n->ops[i + 1].act == lp::ACT_RELU) {
            // output head: both 5x5 depthwise convs and the two-source 1x1 in one launch
            const Op& d2 = n->ops[i + 1];
            const Op& pw = n->ops[i + 2];
            if (lp::launch_headfuse(ptr[o.inA], o.Ca, ptr[d2.inA], d2.Ca, o.wpair_off ? Wt + o.wpair_off : nullptr,
                                    d2.wpair_off ? Wt + d2.wpair_off : nullptr, Wt + pw.w_off, ptr[pw.out], NB, oh, ow,
                                    o.K, pw.Cout, s)) {
                const int64_t px = (int64_t)NB * oh * ow;
                const int rc = prof_mark(o.name.substr(0, o.name.find('.')) == "final_refined"
                                             ? "final." + pw.name.substr(6, pw.name.find('.', 6) - 6) + ".dw5+dw5+pw" : pw.name,
                                         4ll * px * (2ll * o.Ca + 2ll * d2.Ca) + 4ll * px * (o.Ca + d2.Ca + pw.Cout),
                                         2ll * px * ((int64_t)(o.Ca + d2.Ca) * o.K * o.K + (int64_t)(o.Ca + d2.Ca) * pw.Cout),
                                         2ll * px * (int64_t)(o.Ca + d2.Ca) * o.K * o.K);
                if (rc) return rc;
                i += 2;
                continue;
            }
        }
        switch (o.type) {
            case OP_STEM:
                lp::launch_stem(xsrc, Wt + o.w_off, Wt + o.b_off, ptr[o.out], NB, H, W, flip_from, x_batch, s);
                by = 4ll * NB * (3ll * H * W + 32ll * oh * ow);
                fl = 2ll * NB * 32 * 27 * oh * ow;
                break;
            case OP_DW:
                lp::launch_dw(ptr[o.inA], Wt + o.w_off, Wt + o.wdup_off, Wt + o.b_off, ptr[o.out], NB, o.Ca, ih, iw, o.K,
                              o.S, o.act, s);
                by = 4ll * NB * o.Ca * ((int64_t)ih * iw + (int64_t)oh * ow);
                fl = 2ll * NB * o.Ca * o.K * o.K * oh * ow;
                break;
            case OP_PW:
                lp::launch_pw(ptr[o.inA], o.Ca, o.inB >= 0 ? ptr[o.inB] : nullptr, o.Cb, Wt + o.w_off,
                              o.has_bias ? Wt + o.b_off : nullptr, o.res >= 0 ? ptr[o.res] : nullptr,
                              ptr[o.out], NB, oh * ow, o.Cout, o.act, s, o.ws_off ? Wt + o.ws_off : nullptr, n->opt_pw3d);
                by = 4ll * NB * oh * ow * (o.Ca + o.Cb + o.Cout + (o.res >= 0 ? o.Cout : 0));
                fl = 2ll * NB * oh * ow * (int64_t)(o.Ca + o.Cb) * o.Cout;
                break;
            case OP_DECONV: {
                float* inB = o.inB >= 0 ? ptr[o.inB] : nullptr;   // nullptr: the one-source form (plain head)
                if (o.w3_off && deconv4_enabled() && o.w4_off &&
                    lp::launch_deconv4x3(ptr[o.inA], o.Ca, inB, o.Cb, Wt + o.w4_off, Wt + o.b3_off, ptr[o.out], NB,
                                         ih, iw, o.Cout, s)) {
                } else if (o.w3_off && deconv4_enabled())
                    lp::launch_deconv4(ptr[o.inA], o.Ca, inB, o.Cb, Wt + o.w3_off, Wt + o.b3_off, ptr[o.out],
                                       NB, ih, iw, o.Cout, s);
                else if (o.mid == 1)
                    lp::launch_deconv_mfma(ptr[o.inA], o.Ca, inB, o.Cb, Wt + o.w2_off, Wt + o.b2_off,
                                           ptr[o.out], NB, ih, iw, o.Cout, s);
                else
                    lp::launch_deconv_pair(ptr[o.inA], o.Ca, inB, o.Cb, Wt + o.w_off, Wt + o.b_off,
                                           ptr[o.out], NB, ih, iw, o.Cout, s);
                by = 4ll * NB * ((int64_t)(o.Ca + o.Cb) * ih * iw + (int64_t)o.Cout * oh * ow);
                fl = 2ll * NB * (int64_t)(o.Ca + o.Cb) * o.Cout * 4 * oh * ow;
                break;
            }
            case OP_CONVK:
                // dense k x k conv (+ upsample / second source); `oh, ow` already include the stride / the x2
                if (!lp::launch_convk3(o.image_in ? xsrc : ptr[o.inA], o.Ca, o.inB >= 0 ? ptr[o.inB] : nullptr, o.Cb,
                                       Wt + o.wk_off, Wt + o.b_off, ptr[o.out], NB, ih, iw, o.K, o.S, o.ups, o.Cout, o.act,
                                       o.image_in ? flip_from : NB, o.image_in ? x_batch : NB, s))
                    return fail(LP_ERR_UNSUPPORTED, "convk3: shape not supported: " + o.name);
                by = 4ll * NB * ((int64_t)(o.Ca + o.Cb) * ih * iw + (int64_t)o.Cout * oh * ow);
                fl = 2ll * NB * (int64_t)(o.Ca + o.Cb) * o.K * o.K * o.Cout * oh * ow;
                break;
            case OP_DWPW:
                if (!lp::launch_dwpw(ptr[o.inA], Wt + o.w_off, Wt + o.b_off, Wt + o.w2_off, Wt + o.b2_off,
                                     o.res >= 0 ? ptr[o.res] : nullptr, ptr[o.out], NB, o.Ca, ih, iw, o.K, o.S,
                                     o.Cout, s)) {
                    lp::launch_dw(ptr[o.inA], Wt + o.w_off, Wt + o.wdup_off, Wt + o.b_off, ptr[o.mid], NB, o.Ca, ih, iw, o.K,
                                  o.S, lp::ACT_RELU6, s);
                    {
                        const int rc = prof_mark(o.name.substr(0, o.name.find('+')),
                                                 4ll * NB * o.Ca * ((int64_t)ih * iw + (int64_t)oh * ow),
                                                 2ll * NB * o.Ca * o.K * o.K * (int64_t)oh * ow,
                                                 2ll * NB * o.Ca * o.K * o.K * (int64_t)oh * ow);
                        if (rc) return rc;
                    }
                    lp::launch_pw(ptr[o.mid], o.Ca, nullptr, 0, Wt + o.w2_off, Wt + o.b2_off,
                                  o.res >= 0 ? ptr[o.res] : nullptr, ptr[o.out], NB, oh * ow, o.Cout,
                                  lp::ACT_NONE, s, o.ws_off ? Wt + o.ws_off : nullptr, n->opt_pw3d);
                    {
                        const std::string pfx = o.name.substr(0, o.name.rfind('.', o.name.find('+')));
                        const int rc = prof_mark(pfx + ".point_conv",
                                                 4ll * NB * oh * ow * ((int64_t)o.Ca + (int64_t)o.Cout * (o.res >= 0 ? 2 : 1)),
                                                 2ll * NB * oh * ow * (int64_t)o.Ca * o.Cout, 0);
                        if (rc) return rc;
                    }
                    continue;
                }
                // SURVEY 8(d) B_op accounting is per reference op: dw in+out, 1x1 in+out(+res)
                by = 4ll * NB * ((int64_t)o.Ca * ih * iw + 2ll * o.Ca * oh * ow +
                                 (int64_t)o.Cout * oh * ow * (o.res >= 0 ? 2 : 1));
                fl = 2ll * NB * oh * ow * ((int64_t)o.Ca * o.K * o.K + (int64_t)o.Ca * o.Cout);
                break;
        }
        {
            const int rc = prof_mark(o.name, by, fl,
                                     (o.type == OP_STEM || o.type == OP_DW) ? fl
                                     : (o.type == OP_DWPW ? 2ll * NB * oh * ow * (int64_t)o.Ca * o.K * o.K : 0));
            if (rc) return rc;
        }
    }
    return LP_OK;
    };
    if (const int rc = fan_out(n, d_x, N, H, W, flip, s, bptr, esz, run)) return rc;
    HIP_OK(hipGetLastError());
    n->last_ptr.resize(bptr.size());
    for (size_t b = 0; b < bptr.size(); ++b) n->last_ptr[b] = reinterpret_cast<float*>(bptr[b]);
    n->lastN = NB;
    n->lastH = H;
    n->lastW = W;
    return LP_OK;
}

// ---------------------------------------------------------------------------------------------------
// BatchNorm re-calibration of a supernet sub-network (calibrate_test.py:44-122; super_layers.py:19-28)
// ---------------------------------------------------------------------------------------------------
namespace {

size_t calib_part_bytes(const lp_net* n, int N, int H, int W) {
    size_t d = 0;
    for (const auto& L : n->calib->layers) d = std::max(d, lp::bn_partial_doubles(N, L.C, (H / L.div) * (W / L.div)));
    return (d * sizeof(double) + 255) / 256 * 256;
}

}  // namespace

int lp_calib_begin(lp_net* n, double momentum) {
    if (!n) return fail(LP_ERR_INVALID_ARG, "null net");
    if (n->arch.family != 0)
        return fail(LP_ERR_UNSUPPORTED, "calibration: family 0 (pose_mobilenet / pose_simplenet) only");
    if (n->storage != LP_STORAGE_F32) return fail(LP_ERR_UNSUPPORTED, "calibration: fp32 storage only");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(LP_ERR_INVALID_ARG, "momentum must be in [0, 1]");
    for (const auto& t : n->tensors)
        if (!t.is_counter && !t.is_set) return fail(LP_ERR_MISSING_WEIGHT, "missing key in state_dict: " + t.key);
    calib_release(n);
    lp_net* raw = nullptr;
    int rc = lp_net_create(&raw, &n->arch);
    if (rc != LP_OK) return rc;
    raw->tensors = n->tensors;
    raw->identity_fold = true;
    rc = build(*raw);
    if (rc != LP_OK) { lp_net_destroy(raw); return fail(rc, lp_plan::last_error()); }
    auto* c = new lp_net::Calib();
    c->raw = raw;
    c->momentum = momentum;
    auto add = [&](const std::string& key, int C, int div) {
        if (key.empty()) return;
        lp_net::CalibLayer L{key, C, div, arena_push(c->h_bn, 4 * (size_t)C)};
        const char* part[4] = {".weight", ".bias", ".running_mean", ".running_var"};
        for (int q = 0; q < 4; ++q) {
            const Tensor& t = n->tensors[n->index.at(key + part[q])];
            std::copy(t.data.begin(), t.data.end(), c->h_bn.begin() + L.off + (size_t)q * C);
        }
        c->index[key] = (int)c->layers.size();
        c->layers.push_back(L);
    };
    for (const Op& o : raw->ops) {
        if (o.type == OP_DWPW) { add(o.bn0, o.Ca, o.out_div); add(o.bn1, o.Cout, o.out_div); }
        else add(o.bn0, o.type == OP_DW ? o.Ca : o.Cout, o.out_div);
    }
    n->calib = c;
    return LP_OK;
}

size_t lp_calib_workspace_bytes(const lp_net* n, int N, int H, int W) {
    if (!n || !n->calib) { fail(LP_ERR_NOT_FINALIZED, "lp_calib_begin() has not been called"); return 0; }
    const lp_net* raw = n->calib->raw;
    if (N < 1) { fail(LP_ERR_INVALID_ARG, "N must be positive"); return 0; }
    if (check_size(raw, H, W) != LP_OK) return 0;               // lp_last_error names the multiple
    size_t f = 0;
    for (size_t b = 0; b < raw->bufs.ch.size(); ++b) f += buf_floats(raw, (int)b, N, H, W);
    return calib_part_bytes(n, N, H, W) + f * sizeof(float) + 256;
}

int lp_calib_step(lp_net* n, const float* d_x, int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    if (!n || !d_x || !ws) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (!n->calib) return fail(LP_ERR_NOT_FINALIZED, "lp_calib_begin() has not been called");
    lp_net::Calib* c = n->calib;
    lp_net* raw = c->raw;
    if (N < 1) return fail(LP_ERR_INVALID_ARG, "N must be positive");
    if (const int rc = check_size(raw, H, W)) return rc;
    {
        const int m = size_multiple(raw);
        if ((int64_t)N * (H / m) * (W / m) < 2)
            return fail(LP_ERR_INVALID_ARG, "a batch statistic needs more than one value per channel on the deepest plane");
    }
    if (ws_bytes < lp_calib_workspace_bytes(n, N, H, W) || ((uintptr_t)ws & 255))
        return fail(LP_ERR_WORKSPACE, "workspace too small or not 256-byte aligned");
    (void)hipGetLastError();
    if (!c->uploaded) {
        if (!raw->d_weights) {
            HIP_OK(hipMalloc((void**)&raw->d_weights, raw->h_packed.size() * sizeof(float)));
            HIP_OK(hipMemcpy(raw->d_weights, raw->h_packed.data(), raw->h_packed.size() * sizeof(float),
                             hipMemcpyHostToDevice));
        }
        if (!c->d_bn) HIP_OK(hipMalloc((void**)&c->d_bn, c->h_bn.size() * sizeof(float)));
        HIP_OK(hipMemcpy(c->d_bn, c->h_bn.data(), c->h_bn.size() * sizeof(float), hipMemcpyHostToDevice));
        c->uploaded = true;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    std::vector<float*> ptr(raw->bufs.ch.size());
    {
        float* p = (float*)((char*)ws + calib_part_bytes(n, N, H, W));
        for (size_t b = 0; b < ptr.size(); ++b) {
            ptr[b] = p;
            p += buf_floats(raw, (int)b, N, H, W);
        }
    }
    const float* Wt = raw->d_weights;
    lp::launch_notes = false;
    auto bn = [&](const std::string& key, float* x, const float* res, int C, int HW, int act) {
        const lp_net::CalibLayer& L = c->layers[c->index.at(key)];
        lp::launch_bn_stats(x, part, N, C, HW, s);
        lp::launch_bn_apply(x, res, part, c->d_bn + L.off, N, C, HW, act, c->momentum, 1e-5, s);
    };
    for (const Op& o : raw->ops) {
        const int ih = H / o.in_div, iw = W / o.in_div, oh = H / o.out_div, ow = W / o.out_div;
        const std::string &k0 = o.bn0, &k1 = o.bn1;      // the BatchNorm(s) the plan folded into this op
        switch (o.type) {
            case OP_STEM:
                lp::launch_stem_raw(d_x, Wt + o.w_off, ptr[o.out], N, H, W, s);
                bn(k0, ptr[o.out], nullptr, 32, oh * ow, lp::ACT_RELU6);
                break;
            case OP_DW:
                lp::launch_dw(ptr[o.inA], Wt + o.w_off, Wt + o.wdup_off, Wt + o.b_off, ptr[o.out], N, o.Ca, ih, iw, o.K,
                              o.S, lp::ACT_NONE, s);
                bn(k0, ptr[o.out], nullptr, o.Ca, oh * ow, o.act);
                break;
            case OP_PW:
                if (k0.empty()) break;     // the heads' 1x1: behind the last BatchNorm, nothing to calibrate
                lp::launch_pw(ptr[o.inA], o.Ca, nullptr, 0, Wt + o.w_off, Wt + o.b_off, nullptr, ptr[o.out], N, oh * ow,
                              o.Cout, lp::ACT_NONE, s, o.ws_off ? Wt + o.ws_off : nullptr, n->opt_pw3d);
                bn(k0, ptr[o.out], nullptr, o.Cout, oh * ow, o.act);
                break;
            case OP_DWPW:
                lp::launch_dw(ptr[o.inA], Wt + o.w_off, Wt + o.wdup_off, Wt + o.b_off, ptr[o.mid], N, o.Ca, ih, iw, o.K,
                              o.S, lp::ACT_NONE, s);
                bn(k0, ptr[o.mid], nullptr, o.Ca, oh * ow, lp::ACT_RELU6);
                lp::launch_pw(ptr[o.mid], o.Ca, nullptr, 0, Wt + o.w2_off, Wt + o.b2_off, nullptr, ptr[o.out], N, oh * ow,
                              o.Cout, lp::ACT_NONE, s, o.ws_off ? Wt + o.ws_off : nullptr, n->opt_pw3d);
                bn(k1, ptr[o.out], o.res >= 0 ? ptr[o.res] : nullptr, o.Cout, oh * ow, lp::ACT_NONE);
                break;
            case OP_DECONV:
                lp::launch_deconv_raw(ptr[o.inA], o.Ca, o.inB >= 0 ? ptr[o.inB] : nullptr, o.Cb, Wt + o.w_off, ptr[o.out],
                                      N, ih, iw, o.Cout, s);
                bn(k0, ptr[o.out], nullptr, o.Cout, oh * ow, lp::ACT_RELU);
                break;
            default:
                return fail(LP_ERR_UNSUPPORTED, "calibration: op not on the plan: " + o.name);
        }
    }
    HIP_OK(hipGetLastError());
    ++c->steps;
    return LP_OK;
}

int lp_calib_read(const lp_net* n, const char* bn_prefix, float* d_mean, float* d_var, int channels, void* stream) {
    if (!n || !bn_prefix || !d_mean || !d_var) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (!n->calib) return fail(LP_ERR_NOT_FINALIZED, "lp_calib_begin() has not been called");
    const lp_net::Calib* c = n->calib;
    auto it = c->index.find(bn_prefix);
    if (it == c->index.end()) return fail(LP_ERR_UNKNOWN_KEY, std::string("no BatchNorm named ") + bn_prefix);
    const lp_net::CalibLayer& L = c->layers[it->second];
    if (channels != L.C) return fail(LP_ERR_SHAPE, std::string("channel count mismatch for ") + bn_prefix);
    const float* src = c->uploaded ? c->d_bn + L.off : c->h_bn.data() + L.off;
    const hipMemcpyKind kind = c->uploaded ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_OK(hipMemcpyAsync(d_mean, src + 2 * (size_t)L.C, L.C * sizeof(float), kind, (hipStream_t)stream));
    HIP_OK(hipMemcpyAsync(d_var, src + 3 * (size_t)L.C, L.C * sizeof(float), kind, (hipStream_t)stream));
    return LP_OK;
}

int lp_calib_end(lp_net* n, int64_t* steps_out) {
    if (!n) return fail(LP_ERR_INVALID_ARG, "null net");
    if (!n->calib) return fail(LP_ERR_NOT_FINALIZED, "lp_calib_begin() has not been called");
    lp_net::Calib* c = n->calib;
    const int64_t steps = c->steps;
    if (c->uploaded) {
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(c->h_bn.data(), c->d_bn, c->h_bn.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (const auto& L : c->layers) {
            Tensor& m = n->tensors[n->index.at(L.bn + ".running_mean")];
            Tensor& v = n->tensors[n->index.at(L.bn + ".running_var")];
            std::copy(c->h_bn.begin() + L.off + 2 * (size_t)L.C, c->h_bn.begin() + L.off + 3 * (size_t)L.C, m.data.begin());
            std::copy(c->h_bn.begin() + L.off + 3 * (size_t)L.C, c->h_bn.begin() + L.off + 4 * (size_t)L.C, v.data.begin());
        }
    }
    calib_release(n);
    if (steps_out) *steps_out = steps;
    if (steps > 0) return lp_net_finalize(n, 1);
    return LP_OK;
}

// the op whose output is published as `name` (a tap name or an op name); the heads' 1x1 of a 16-bit plan are the fp32
// outputs the caller owns, not taps
static const OpBase* find_tap(const lp_net* n, const char* name) {
    const OpBase* hit = nullptr;
    auto match = [&](const OpBase& o) { if (!hit && (o.tap == name || o.name == name)) hit = &o; };
    for (const Op& o : n->ops) match(o);                       // a built plan fills one of the two lists
    for (const BOp& o : n->bops) if (!o.out_f32) match(o);
    return hit;
}

int64_t lp_net_tap(const lp_net* n, const char* name, float* d_dst, void* stream) {
    if (!n || !name || n->last_ptr.empty()) return fail(LP_ERR_INVALID_ARG, "no forward has run");
    const OpBase* o = find_tap(n, name);
    if (!o) return fail(LP_ERR_UNKNOWN_KEY, std::string("unknown tap ") + name);
    const int d = n->bufs.div[o->out];
    const int hw = (n->lastH / d) * (n->lastW / d);
    const int64_t cnt = (int64_t)n->lastN * n->bufs.ch[o->out] * hw;
    if (n->storage != LP_STORAGE_F32) {
        if ((size_t)o->out >= n->last_stored_b.size() || !n->last_stored_b[o->out])
            return fail(LP_ERR_UNSUPPORTED, std::string("tap ") + name + ": the last forward did not store this "
                        "tensor (it lives inside a fused block launch; option \"mbtb\" = 0 runs one launch per op)");
        if (d_dst)
            lp::launch_octet_to_planar(n->last_ptr_b[o->out], d_dst, n->lastN, n->bufs.ch[o->out], hw,
                                       (hipStream_t)stream, n->storage == LP_STORAGE_F16);
    } else if (d_dst) {
        hipError_t e = hipMemcpyAsync(d_dst, n->last_ptr[o->out], (size_t)cnt * sizeof(float),
                                      hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(LP_ERR_HIP, hipGetErrorString(e));
    }
    return cnt;
}

int64_t lp_net_tap_offset(const lp_net* n, const char* name, int NB, int H, int W, int64_t* count) {
    if (!n || !name || !n->finalized) return fail(LP_ERR_INVALID_ARG, "net not finalized");
    if (n->storage != LP_STORAGE_F32) return fail(LP_ERR_UNSUPPORTED, "fp32 storage only");
    if (NB < 1) return fail(LP_ERR_INVALID_ARG, "NB must be positive");
    if (const int rc = check_size(n, H, W)) return rc;
    const OpBase* o = find_tap(n, name);
    if (!o) return fail(LP_ERR_UNKNOWN_KEY, std::string("unknown tap ") + name);
    if (o->out == n->out0_buf || o->out == n->out1_buf) return fail(LP_ERR_UNSUPPORTED, "caller-owned output");
    size_t off = 0;
    for (int b = 0; b < o->out; ++b) off += buf_floats(n, b, NB, H, W);
    const int d = n->bufs.div[o->out];
    if (count) *count = (int64_t)NB * n->bufs.ch[o->out] * (H / d) * (W / d);
    return (int64_t)(off * sizeof(float));
}

int lp_net_set_storage(lp_net* n, int storage) {
    if (!n || (storage != LP_STORAGE_F32 && storage != LP_STORAGE_BF16 && storage != LP_STORAGE_F16))
        return fail(LP_ERR_INVALID_ARG, "storage must be LP_STORAGE_F32, LP_STORAGE_BF16 or LP_STORAGE_F16");
    if (n->calib) return fail(LP_ERR_INVALID_ARG, "a calibration is open on this handle: lp_calib_end() first");
    if (n->arch.family == 1 && storage != LP_STORAGE_F32)
        return fail(LP_ERR_UNSUPPORTED, "lp_net_set_storage: the pose_resnet family (lp_arch.family = 1) runs in fp32 storage "
                                        "only: its dense k x k convolutions have no 16-bit kernels yet");
    if (storage != n->storage) {
        n->storage = storage;
        n->finalized = false;
        n->last_ptr.clear();
    }
    return LP_OK;
}

int lp_net_get_storage(const lp_net* n) { return n ? n->storage : LP_ERR_INVALID_ARG; }

int lp_round16(const float* src, float* dst, int64_t count, int storage) {
    if ((!src || !dst) && count > 0) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (storage != LP_STORAGE_BF16 && storage != LP_STORAGE_F16)
        return fail(LP_ERR_INVALID_ARG, "storage must be LP_STORAGE_BF16 or LP_STORAGE_F16");
    for (int64_t i = 0; i < count; ++i) dst[i] = round16(storage, src[i]);
    return LP_OK;
}

typedef lp_net::OptEntryT OptEntry;
const std::vector<OptEntry>& lp_net::options() {
    static const std::vector<OptEntry> t = {
        {"mb16", 0, 1, &lp_net::opt_mb16},
        {"mb16_run", 0, 1, &lp_net::opt_mb16_run},
        {"mb16_min", 0, 65536, &lp_net::opt_mb16_min},
        {"mbt", 0, 3, &lp_net::opt_mbt},
        {"mbt_s2", 0, 1, &lp_net::opt_mbt_s2},
        {"mbconv2", 0, 1, &lp_net::opt_mbconv2},
        {"mbtb", 0, 1, &lp_net::opt_mbtb},
        {"mbtb_s2", 0, 1, &lp_net::opt_mbtb_s2},
        {"mbtq", 0, 2, &lp_net::opt_mbtq},
        {"mbtd", 0, 1, &lp_net::opt_mbtd},
        {"pw3d", 0, 2, &lp_net::opt_pw3d},
        {"headb", 0, 1, &lp_net::opt_headb},
        {"headfuse", 0, 1, &lp_net::opt_headfuse},
        {"dwt", 0, 2, &lp_net::opt_dwt},
        {"stem", 0, 1, &lp_net::opt_stem},
        {"diag_dwpw", 0, 2, &lp_net::opt_diag_dwpw},
    };
    return t;
}

int lp_net_set_option(lp_net* n, const char* key, int value) {
    if (!n || !key) return fail(LP_ERR_INVALID_ARG, "null argument");
    for (const OptEntry& e : lp_net::options())
        if (!strcmp(key, e.key)) {
            if (value < e.lo || value > e.hi) return fail(LP_ERR_INVALID_ARG, std::string("option ") + key + ": value out of range");
#ifndef LP_DIAG_BUILD
            if (e.field == &lp_net::opt_diag_dwpw && value != 0)
                return fail(LP_ERR_UNSUPPORTED, "option diag_dwpw: the self-checking dwpw_kernel exists only in the diagnostics "
                                                "flavour of the library (python -m litepose_amd.build --flavour diag, "
                                                "LP_NATIVE_FLAVOUR=diag)");
#endif
            n->*(e.field) = value;
            return LP_OK;
        }
    return fail(LP_ERR_UNKNOWN_KEY, std::string("unknown option ") + key);
}

int lp_net_get_option(const lp_net* n, const char* key) {
    if (!n || !key) return fail(LP_ERR_INVALID_ARG, "null argument");
    for (const OptEntry& e : lp_net::options())
        if (!strcmp(key, e.key)) return n->*(e.field);
    return fail(LP_ERR_UNKNOWN_KEY, std::string("unknown option ") + key);
}

int lp_diag_read(uint32_t* words, int cap_words, int clear) {
    const int n = lp::dwpw_diag_read(words, cap_words, clear != 0);
    if (n == -2) return fail(LP_ERR_UNSUPPORTED, "lp_diag_read: no diagnostic kernel in this library (build --flavour diag)");
    if (n < 0) return fail(LP_ERR_HIP, "lp_diag_read: copy from the device log failed");
    return n;
}

int lp_phase_trace_read(uint64_t* words, int nwg) {
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    const int n = lp::phase_trace_read(reinterpret_cast<unsigned long long*>(words), nwg);
    if (n == -2) return fail(LP_ERR_UNSUPPORTED, "lp_phase_trace_read: no phase trace in this library (build --flavour trace)");
    if (n < 0) return fail(LP_ERR_HIP, "lp_phase_trace_read: bad count / copy from the device table failed");
    return n;
}

int lp_wg_trace_read(uint64_t* words, int nwg, int select_cexp) {
    if (nwg < 0 || nwg > 16384) return fail(LP_ERR_INVALID_ARG, "lp_wg_trace_read: 0..16384 workgroups");
    const int n = lp::wg_trace_read(reinterpret_cast<unsigned long long*>(words), nwg, select_cexp);
    if (n == -2) return fail(LP_ERR_UNSUPPORTED, "lp_wg_trace_read: no trace in this library (build --flavour trace)");
    if (n < 0) return fail(LP_ERR_HIP, "lp_wg_trace_read: copy failed");
    return n;
}

int lp_net_set_streams(lp_net* n, int k) {
    if (!n || k < 1 || k > lp_net::MAX_SIDE) return fail(LP_ERR_INVALID_ARG, "streams must be 1..8");
    n->nstreams = k;
    return LP_OK;
}

int lp_net_set_profiling(lp_net* n, int enable) {
    if (!n) return fail(LP_ERR_INVALID_ARG, "null net");
    n->profiling = enable != 0;
    return LP_OK;
}

int lp_net_profile(const lp_net* n, char names[][48], float* ms, int64_t* alg_bytes, int64_t* flops,
                   int cap) {
    return lp_net_profile2(n, names, ms, alg_bytes, flops, nullptr, cap);
}

int lp_net_profile2(const lp_net* n, char names[][48], float* ms, int64_t* alg_bytes, int64_t* flops,
                    int64_t* flops_valu, int cap) {
    if (!n || !n->profiling || n->prof_entries.empty())
        return fail(LP_ERR_INVALID_ARG, "profiling not enabled / no forward yet");
    if (hipEventSynchronize(n->events[n->prof_ev]) != hipSuccess)
        return fail(LP_ERR_HIP, "hipEventSynchronize failed");
    const int cnt = std::min((int)n->prof_entries.size(), cap);
    for (int i = 0; i < cnt; ++i) {
        const auto& e = n->prof_entries[i];
        float t = 0.f;
        (void)hipEventElapsedTime(&t, n->events[e.ev0], n->events[e.ev1]);
        if (ms) ms[i] = t;
        if (alg_bytes) alg_bytes[i] = e.bytes;
        if (flops) flops[i] = e.flops;
        if (flops_valu) flops_valu[i] = e.flops_valu;
        if (names) {
            // "<op name>|<kernel>"; the op name is shortened if needed so the kernel tag survives
            std::string nm = e.name;
            if (nm.size() + e.kernel.size() + 1 > 47) nm = nm.substr(0, 46 - e.kernel.size());
            nm += "|" + e.kernel;
            std::strncpy(names[i], nm.c_str(), 47);
            names[i][47] = 0;
        }
    }
    return cnt;
}

}  // extern "C"
