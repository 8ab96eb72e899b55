// C ABI of the training-mode layers (include/litepose_amd.h, "training-mode layers"): argument validation and workspace
// carving; the kernels live in layer_kernels.hip, the 1x1 and depthwise forwards are the network's own launch_pw / launch_dw.
#include <hip/hip_runtime.h>

#include "../../include/litepose_amd.h"
#include "kernels.h"

extern "C" void lp_set_error_(const char* msg);   // engine.cpp owns the thread-local slot

namespace {
int fail(int code, const char* msg) {
    lp_set_error_(msg);
    return code;
}
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool big(long long v) { return v > 0x7fffff00LL; }       // 2^31 - 256: index loops look a few steps ahead
// floats of launch_pw's A fragments of an [M][K] weight, and of its zero bias
size_t frag_floats(int M, int K) { return (size_t)((M + 31) / 32) * ((K + 1) / 2) * 64; }
size_t bias_floats(int M) { return (size_t)((M + 31) / 32) * 32; }
bool dw_shape_ok(int K, int S) { return (K == 3 || K == 5 || K == 7) && (S == 1 || S == 2); }
}  // namespace

extern "C" {

size_t lp_bn_workspace_bytes(int N, int C, int HW) {
    if (N < 1 || C < 1 || HW < 1 || C > 65535 || big((long long)N * HW) || big((long long)C * HW)) return 0;
    return lp::bn_partial_doubles(N, C, HW) * sizeof(double);
}

static int bn_check(int N, int C, int HW, int act) {
    if (N < 1 || C < 1 || HW < 1) return fail(LP_ERR_INVALID_ARG, "N, C and HW must be positive");
    if (act < 0 || act > 2) return fail(LP_ERR_INVALID_ARG, "act must be 0 (none), 1 (ReLU) or 2 (ReLU6)");
    if (C > 65535 || big((long long)N * HW) || big((long long)C * HW))
        return fail(LP_ERR_UNSUPPORTED, "C must be <= 65535, N * HW and C * HW at most 2^31 - 256");
    return LP_OK;
}

int lp_bn_forward(const float* d_x, const float* d_gamma, const float* d_beta, float* running_io, const float* d_res,
                  float* y_out, double* stat_out, int N, int C, int HW, int act, int training, double momentum, double eps,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = bn_check(N, C, HW, act)) return rc;
    if (!d_x || !d_gamma || !d_beta || !running_io || !y_out) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (training && !stat_out) return fail(LP_ERR_INVALID_ARG, "a training-mode forward needs stat_out");
    if (!(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return fail(LP_ERR_INVALID_ARG, "eps >= 0, momentum in [0, 1]");
    if (!al16(d_x) || !al16(y_out) || !al16(d_res)) return fail(LP_ERR_INVALID_ARG, "x, res and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (training) {
        if (!workspace || workspace_bytes < lp_bn_workspace_bytes(N, C, HW)) return fail(LP_ERR_WORKSPACE, "bn workspace too small");
        if (!al16(workspace) || ((uintptr_t)stat_out & 7)) return fail(LP_ERR_WORKSPACE, "bn workspace must be 16-byte, stat_out 8-byte aligned");
        lp::launch_bn_stats(d_x, (double*)workspace, N, C, HW, s);
    }
    lp::launch_bn_fwd(d_x, d_res, (const double*)workspace, d_gamma, d_beta, running_io, y_out, stat_out, N, C, HW, act,
                      training != 0, momentum, eps, s);
    if (hipGetLastError() != hipSuccess) return fail(LP_ERR_HIP, "bn_forward launch failed");
    return LP_OK;
}

int lp_bn_backward(const float* d_grad_y, const float* d_x, const float* d_gamma, const float* d_beta, const double* d_stat,
                   float* grad_x_out, float* grad_gamma_out, float* grad_beta_out, int N, int C, int HW, int act,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = bn_check(N, C, HW, act)) return rc;
    if (!d_grad_y || !d_x || !d_gamma || !d_beta || !d_stat || !grad_x_out || !grad_gamma_out || !grad_beta_out)
        return fail(LP_ERR_INVALID_ARG, "null argument");
    if (!al16(d_grad_y) || !al16(d_x) || !al16(grad_x_out) || ((uintptr_t)d_stat & 7))
        return fail(LP_ERR_INVALID_ARG, "grad_y, x and grad_x must be 16-byte, stat 8-byte aligned");
    if (!workspace || workspace_bytes < lp_bn_workspace_bytes(N, C, HW)) return fail(LP_ERR_WORKSPACE, "bn workspace too small");
    if (!al16(workspace)) return fail(LP_ERR_WORKSPACE, "bn workspace must be 16-byte aligned");
    lp::launch_bn_bwd(d_grad_y, d_x, d_gamma, d_beta, d_stat, (double*)workspace, grad_x_out, grad_gamma_out, grad_beta_out,
                      N, C, HW, act, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(LP_ERR_HIP, "bn_backward launch failed");
    return LP_OK;
}

static int pw_check(int N, int Cin, int Cout, int HW) {
    if (N < 1 || Cin < 1 || Cout < 1 || HW < 1) return fail(LP_ERR_INVALID_ARG, "N, Cin, Cout and HW must be positive");
    if (Cin > 65535 || Cout > 65535 || big((long long)N * HW) || big((long long)Cin * HW) || big((long long)Cout * HW))
        return fail(LP_ERR_UNSUPPORTED, "channels must be <= 65535, N * HW and C * HW at most 2^31 - 256");
    return LP_OK;
}

size_t lp_pw_forward_workspace_bytes(int Cin, int Cout) {
    if (Cin < 1 || Cout < 1 || Cin > 65535 || Cout > 65535) return 0;
    return (frag_floats(Cout, Cin) + bias_floats(Cout)) * sizeof(float);
}

int lp_pw_forward(const float* d_x, const float* d_w, float* y_out, int N, int Cin, int Cout, int HW, void* workspace,
                  size_t workspace_bytes, void* stream) {
    if (int rc = pw_check(N, Cin, Cout, HW)) return rc;
    if (!d_x || !d_w || !y_out) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (!al16(d_x) || !al16(y_out)) return fail(LP_ERR_INVALID_ARG, "x and y must be 16-byte aligned");
    if (!workspace || workspace_bytes < lp_pw_forward_workspace_bytes(Cin, Cout)) return fail(LP_ERR_WORKSPACE, "pw workspace too small");
    if (!al16(workspace)) return fail(LP_ERR_WORKSPACE, "pw workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* wp = (float*)workspace;
    float* zb = wp + frag_floats(Cout, Cin);
    lp::launch_pw_pack(d_w, Cout, Cin, false, wp, zb, s);
    lp::launch_pw(d_x, Cin, nullptr, 0, wp, zb, nullptr, y_out, N, HW, Cout, lp::ACT_NONE, s);
    if (hipGetLastError() != hipSuccess) return fail(LP_ERR_HIP, "pw_forward launch failed");
    return LP_OK;
}

size_t lp_pw_backward_workspace_bytes(int N, int Cin, int Cout, int HW, int want_x, int want_w) {
    if (N < 1 || Cin < 1 || Cout < 1 || HW < 1 || Cin > 65535 || Cout > 65535 || big((long long)N * HW)) return 0;
    size_t fl = 0;
    if (want_x) fl += frag_floats(Cin, Cout) + bias_floats(Cin);
    if (want_w) fl += (size_t)lp::pw_wgrad_slices((long)N * HW) * Cout * Cin;
    return fl * sizeof(float);
}

int lp_pw_backward(const float* d_grad_y, const float* d_x, const float* d_w, float* grad_x_out, float* grad_w_out, int N,
                   int Cin, int Cout, int HW, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = pw_check(N, Cin, Cout, HW)) return rc;
    if (!d_grad_y || (!grad_x_out && !grad_w_out)) return fail(LP_ERR_INVALID_ARG, "null argument / no output requested");
    if (grad_x_out && !d_w) return fail(LP_ERR_INVALID_ARG, "grad_x_out needs d_w");
    if (grad_w_out && !d_x) return fail(LP_ERR_INVALID_ARG, "grad_w_out needs d_x");
    if (!al16(d_grad_y) || !al16(d_x) || !al16(grad_x_out)) return fail(LP_ERR_INVALID_ARG, "grad_y, x and grad_x must be 16-byte aligned");
    if (!workspace || workspace_bytes < lp_pw_backward_workspace_bytes(N, Cin, Cout, HW, grad_x_out != nullptr, grad_w_out != nullptr))
        return fail(LP_ERR_WORKSPACE, "pw workspace too small");
    if (!al16(workspace)) return fail(LP_ERR_WORKSPACE, "pw workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (grad_x_out) {
        float* wp = ws;
        float* zb = wp + frag_floats(Cin, Cout);
        ws = zb + bias_floats(Cin);
        lp::launch_pw_pack(d_w, Cout, Cin, true, wp, zb, s);
        lp::launch_pw(d_grad_y, Cout, nullptr, 0, wp, zb, nullptr, grad_x_out, N, HW, Cin, lp::ACT_NONE, s);
    }
    if (grad_w_out) lp::launch_pw_wgrad(d_grad_y, d_x, ws, grad_w_out, N, HW, Cout, Cin, s);
    if (hipGetLastError() != hipSuccess) return fail(LP_ERR_HIP, "pw_backward launch failed");
    return LP_OK;
}

static int dw_check(int N, int C, int H, int W, int K, int S) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail(LP_ERR_INVALID_ARG, "N, C, H and W must be positive");
    if (!dw_shape_ok(K, S)) return fail(LP_ERR_UNSUPPORTED, "K must be 3, 5 or 7 and S 1 or 2");
    if (S == 2 && ((H | W) & 1)) return fail(LP_ERR_INVALID_ARG, "stride 2 is defined for even H and W only");
    if (H > 16384 || W > 16384 || big((long long)N * C * ((H + 15) / 16) * ((W + 15) / 16)) || big((long long)C * K * K))
        return fail(LP_ERR_UNSUPPORTED, "H, W <= 16384 and N * C * (16x16 tiles of a plane) below 2^31");
    return LP_OK;
}

size_t lp_dw_forward_workspace_bytes(int C, int K) {
    if (C < 1 || (K != 3 && K != 5 && K != 7) || big((long long)C * K * K)) return 0;
    return ((size_t)2 * C * K * K + C) * sizeof(float);
}

int lp_dw_forward(const float* d_x, const float* d_w, float* y_out, int N, int C, int H, int W, int K, int S,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = dw_check(N, C, H, W, K, S)) return rc;
    if (!d_x || !d_w || !y_out) return fail(LP_ERR_INVALID_ARG, "null argument");
    if (!al16(d_x) || !al16(y_out)) return fail(LP_ERR_INVALID_ARG, "x and y must be 16-byte aligned");
    if (!workspace || workspace_bytes < lp_dw_forward_workspace_bytes(C, K)) return fail(LP_ERR_WORKSPACE, "dw workspace too small");
    if (!al16(workspace)) return fail(LP_ERR_WORKSPACE, "dw workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* wdup = (float*)workspace;
    float* zb = wdup + (size_t)2 * C * K * K;
    lp::launch_dw_pack(d_w, C, K, wdup, zb, s);
    lp::launch_dw(d_x, d_w, wdup, zb, y_out, N, C, H, W, K, S, lp::ACT_NONE, s);
    if (hipGetLastError() != hipSuccess) return fail(LP_ERR_HIP, "dw_forward launch failed");
    return LP_OK;
}

size_t lp_dw_backward_workspace_bytes(int N, int C, int H, int W, int K, int S, int want_w) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || !dw_shape_ok(K, S) || (S == 2 && ((H | W) & 1)) || H > 16384 || W > 16384) return 0;
    if (!want_w) return 0;
    return (size_t)lp::dw_wgrad_slices(N, (H - 1) / S + 1, (W - 1) / S + 1) * C * K * K * sizeof(float);
}

int lp_dw_backward(const float* d_grad_y, const float* d_x, const float* d_w, float* grad_x_out, float* grad_w_out, int N,
                   int C, int H, int W, int K, int S, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = dw_check(N, C, H, W, K, S)) return rc;
    if (C > 65535) return fail(LP_ERR_UNSUPPORTED, "C must be <= 65535");
    if (!d_grad_y || (!grad_x_out && !grad_w_out)) return fail(LP_ERR_INVALID_ARG, "null argument / no output requested");
    if (grad_x_out && !d_w) return fail(LP_ERR_INVALID_ARG, "grad_x_out needs d_w");
    if (grad_w_out && !d_x) return fail(LP_ERR_INVALID_ARG, "grad_w_out needs d_x");
    if (grad_w_out) {
        if (!workspace || workspace_bytes < lp_dw_backward_workspace_bytes(N, C, H, W, K, S, 1))
            return fail(LP_ERR_WORKSPACE, "dw workspace too small");
        if ((uintptr_t)workspace & 3) return fail(LP_ERR_WORKSPACE, "dw workspace must be 4-byte aligned");
    }
    lp::launch_dw_backward(d_grad_y, d_x, d_w, grad_x_out, (float*)workspace, grad_w_out, N, C, H, W, K, S,
                           (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(LP_ERR_HIP, "dw_backward launch failed");
    return LP_OK;
}

}  // extern "C"
