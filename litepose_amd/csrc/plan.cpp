// Host half of lp_net_finalize (plan.h): architecture bookkeeping, BatchNorm folding, weight packing and the op / buffer
// lists of one LitePose forward.  Plain C++: nothing here touches the device.
//
// One walk() owns the topology -- stem, stages, three deconvs with an output head after the second and the third -- and
// with it the raw-source indices, the op and tap names and the refusals.  Three forms supply the emitters it calls (stem,
// block, deconv, head): Family0<F32> and Family0<B16> (fp32 and 16-bit storage) and Resnet (family 1).  TWO THINGS ARE
// FIXED and tests/test_plan_cpu.py pins them: the order in which the emitters call new_buf (buffer ids lay out the
// workspace and are what lp_net_tap_offset returns) and the order of every arena_push (offsets and padding of h_packed).
//
// Reference code this replaces (nothing is copied; semantics only):
//   lib/models/pose_mobilenet.py:12-19    _make_divisible
//   lib/models/pose_mobilenet.py:22-71    LitePose.__init__ (channel bookkeeping)
//   lib/models/pose_mobilenet.py:86-135   head / deconv construction
//   lib/models/pose_mobilenet.py:137-156  forward (op order below)
//   fuse_bn.py:81-137,147-162             BN folding algebra
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace lp_plan {

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int make_divisible(double v, int divisor) {
    int nv = std::max(divisor, (int)(v + divisor / 2.0) / divisor * divisor);
    if (nv < 0.9 * v) nv += divisor;
    return nv;
}

void add_tensor(Net& n, const std::string& key, std::vector<int64_t> shape, bool counter = false) {
    Tensor t;
    t.key = key;
    t.shape = std::move(shape);
    t.is_counter = counter;
    n.index[key] = (int)n.tensors.size();
    n.tensors.push_back(std::move(t));
}
void add_bn(Net& n, const std::string& p, int c) {
    add_tensor(n, p + ".weight", {c});
    add_tensor(n, p + ".bias", {c});
    add_tensor(n, p + ".running_mean", {c});
    add_tensor(n, p + ".running_var", {c});
    add_tensor(n, p + ".num_batches_tracked", {}, true);
}
const Tensor& T(const Net& n, const std::string& key) { return n.tensors[n.index.at(key)]; }

// BN (eval) -> per-channel scale / shift:  y = x*scale + shift.  The op the BatchNorm is folded into records its key
// (launch order: bn0, then bn1) -- what calibration makes its layer list from
void bn_fold(const Net& n, OpBase& op, const std::string& p, std::vector<double>& scale, std::vector<double>& shift) {
    (op.bn0.empty() ? op.bn0 : op.bn1) = p;
    const Tensor &g = T(n, p + ".weight"), &b = T(n, p + ".bias");
    const Tensor &m = T(n, p + ".running_mean"), &v = T(n, p + ".running_var");
    const size_t c = g.data.size();
    if (n.identity_fold) {                 // calibration plan: the conv's own weights, BatchNorm applied by bn_apply_kernel
        scale.assign(c, 1.0);
        shift.assign(c, 0.0);
        return;
    }
    scale.resize(c);
    shift.resize(c);
    for (size_t i = 0; i < c; ++i) {
        const double s = (double)g.data[i] / std::sqrt((double)v.data[i] + 1e-5);
        scale[i] = s;
        shift[i] = (double)b.data[i] - (double)m.data[i] * s;
    }
}

int new_buf(Net& n, int ch, int div) {
    n.bufs.ch.push_back(ch);
    n.bufs.div.push_back(div);
    return (int)n.bufs.ch.size() - 1;
}

// ---------------------------------------------------------------------------------------------------
// Shared packing helpers.  arena_push may move h_packed, so no helper hands out a pointer into it: a push_* helper
// pushes its own block, derives the pointer AFTER the push, fills the block and returns the block's offset; the values
// it is given read the arena by offset.
// ---------------------------------------------------------------------------------------------------

// exact 3-way bf16 split: x == hi + mid + lo, each a bf16 (truncation; the remainders are exact)
inline void split3(float x, uint32_t out[3]) {
    for (int t = 0; t < 3; ++t) {
        uint32_t u;
        std::memcpy(&u, &x, 4);
        u &= 0xffff0000u;
        float h;
        std::memcpy(&h, &u, 4);
        out[t] = u >> 16;
        x = x - h;                       // exact
    }
}

uint16_t bf16_rne(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// IEEE half: the compiler's float -> _Float16 conversion rounds to nearest even, overflows to +-inf and keeps
// subnormals (as tensor.to(torch.float16) does); tests/test_f16_cpu.py checks it through lp_round16.  The float is read
// through a volatile: inlined into a caller that computes it as (float)(double), clang folds double -> float -> half
// into ONE double -> half conversion (__truncdfhf2), which rounds a folded weight that is an exact fp16 tie as a float
// the other way than torch's .to(float16) of the float does (double rounding is not rounding)
uint16_t f16_rne(float x) {
    volatile float v = x;
    const _Float16 h = (_Float16)v;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}
// the bits of one 16-bit record element in the net's storage format
uint16_t rne16(const Net& n, float x) { return n.storage == LP_STORAGE_F16 ? f16_rne(x) : bf16_rne(x); }
const char* storage_name(const Net& n) { return n.storage == LP_STORAGE_F16 ? "f16" : "bf16"; }

// A fragments of v_mfma_f32_32x32x16_bf16 as exact bf16x3 pieces: [cblock][step][piece hi,mid,lo][64 lanes][4 dwords];
// lane l holds row co = cb*32 + (l&31) and k = step*16 + 8*(l>>5) + 0..7 (two bf16 per dword, even k in the low half).
// value(co, k) -> float, zero where the operand is padding
template <class V>
size_t push_afrag3(Net& n, int cblocks, int steps, V value) {
    const size_t off = arena_push(n.h_packed, (size_t)cblocks * steps * 3 * 64 * 4);
    uint32_t* d = reinterpret_cast<uint32_t*>(n.h_packed.data() + off);
    for (int cb = 0; cb < cblocks; ++cb)
        for (int st = 0; st < steps; ++st)
            for (int l = 0; l < 64; ++l) {
                uint32_t piece[8][3];
                for (int e = 0; e < 8; ++e) split3(value(cb * 32 + (l & 31), st * 16 + 8 * (l >> 5) + e), piece[e]);
                for (int pc = 0; pc < 3; ++pc)
                    for (int dq = 0; dq < 4; ++dq)
                        d[((((size_t)cb * steps + st) * 3 + pc) * 64 + l) * 4 + dq] =
                            piece[2 * dq][pc] | (piece[2 * dq + 1][pc] << 16);
            }
    return off;
}
// the same fragments with one 16-bit value (the net's storage format, round-to-nearest-even): [cblock][step][64][4]
template <class V>
size_t push_afrag16(Net& n, int cblocks, int steps, V value) {
    const size_t off = arena_push(n.h_packed, (size_t)cblocks * steps * 64 * 4);
    uint32_t* d = reinterpret_cast<uint32_t*>(n.h_packed.data() + off);
    for (int cb = 0; cb < cblocks; ++cb)
        for (int st = 0; st < steps; ++st)
            for (int l = 0; l < 64; ++l)
                for (int dq = 0; dq < 4; ++dq) {
                    const int co = cb * 32 + (l & 31), k = st * 16 + 8 * (l >> 5) + 2 * dq;
                    d[(((size_t)cb * steps + st) * 64 + l) * 4 + dq] =
                        (uint32_t)rne16(n, value(co, k)) | ((uint32_t)rne16(n, value(co, k + 1)) << 16);
                }
    return off;
}
// fp32 A fragments of v_mfma_f32_32x32x2_f32: [block][K/2][64 lanes]; lane l holds row l&31 and k = 2*kp + (l>>5).
// value(block, row, k)
template <class V>
size_t push_afrag32(Net& n, int blocks, int KP, V value) {
    const size_t off = arena_push(n.h_packed, (size_t)blocks * KP * 64);
    float* d = n.h_packed.data() + off;
    for (int blk = 0; blk < blocks; ++blk)
        for (int kp = 0; kp < KP; ++kp)
            for (int l = 0; l < 64; ++l) d[((size_t)blk * KP + kp) * 64 + l] = value(blk, l & 31, 2 * kp + (l >> 5));
    return off;
}
// bias in D-fragment order [cblock][half][16]: entry (half, r) belongs to channel cb*32 + 4*half + (r&3) + 8*(r>>2);
// zeros when the layer has no bias (shift = nullptr) / for padding rows
size_t push_bias_dfrag(Net& n, int cblocks, int Cout, const std::vector<double>* shift) {
    const size_t off = arena_push(n.h_packed, (size_t)cblocks * 32);
    for (int cb = 0; cb < cblocks; ++cb)
        for (int half = 0; half < 2; ++half)
            for (int r = 0; r < 16; ++r) {
                const int co = cb * 32 + 4 * half + (r & 3) + 8 * (r >> 2);
                n.h_packed[off + ((size_t)cb * 2 + half) * 16 + r] = (shift && co < Cout) ? (float)(*shift)[co] : 0.f;
            }
    return off;
}
size_t push_bias(Net& n, const std::vector<double>& shift) {
    const size_t off = arena_push(n.h_packed, shift.size());
    for (size_t c = 0; c < shift.size(); ++c) n.h_packed[off + c] = (float)shift[c];
    return off;
}

// transposed conv 4x4 s2: output parity par = 2a + b takes 2 x 2 of the 16 taps, in the order the kernels walk them:
// a = 0: ky {1, 3}, a = 1: ky {0, 2} (same for b / kx); t = 0..3 -> tap index ky*4 + kx
inline int deconv_tap(int par, int t) {
    const int ky = 1 - (par >> 1) + 2 * (t >> 1), kx = 1 - (par & 1) + 2 * (t & 1);
    return ky * 4 + kx;
}

// 7x7 depthwise filters as the fused block kernels read them, a filter row of a channel pair as four 16-byte LDS words:
// [npairs][7 rows][7 taps x 2 ch, 2 pad floats]; the pad of row 0 carries the pair's bias; pairs beyond C stay zero.
// at(c, t): arena offset of tap t = ky*7 + kx of channel c, t = 49: of its bias
template <class At>
size_t push_pair_rows(Net& n, int npairs, int C, At at) {
    const size_t off = arena_push(n.h_packed, (size_t)npairs * 7 * 16);
    for (int c = 0; c < C; ++c) {
        for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx)
                n.h_packed[off + ((size_t)(c >> 1) * 7 + ky) * 16 + 2 * kx + (c & 1)] = n.h_packed[at(c, ky * 7 + kx)];
        n.h_packed[off + (size_t)(c >> 1) * 7 * 16 + 14 + (c & 1)] = n.h_packed[at(c, 49)];
    }
    return off;
}

// the fused stem's copies of the three folded weight sets (stem3_kernel / stem4_kernel<F, C0>): conv tap-major
// [27][32], depthwise tap-major [9][32] (+ its bias [32] when with_b1), 1x1 input-major [32][c0] + bias [c0].
// dw_at(c, t): arena offset of depthwise tap t of channel c (t = 9: its bias); rnd: the rounding of the 1x1 weights
template <class At, class Rnd>
void pack_fused_stem(Net& n, OpBase& st, At dw_at, bool with_b1, const std::vector<double>& sc,
                     const std::vector<double>& sh, Rnd rnd) {
    const int c0 = n.c0;
    st.st_w0 = arena_push(n.h_packed, 27 * 32);
    for (int co = 0; co < 32; ++co)
        for (int t = 0; t < 27; ++t) n.h_packed[st.st_w0 + t * 32 + co] = n.h_packed[st.w_off + co * 27 + t];
    st.st_w1 = arena_push(n.h_packed, 9 * 32);
    if (with_b1) st.st_b1 = arena_push(n.h_packed, 32);
    for (int c = 0; c < 32; ++c) {
        for (int t = 0; t < 9; ++t) n.h_packed[st.st_w1 + t * 32 + c] = n.h_packed[dw_at(c, t)];
        if (with_b1) n.h_packed[st.st_b1 + c] = n.h_packed[dw_at(c, 9)];
    }
    const Tensor& w2 = T(n, "first.2.weight");
    st.st_w2 = arena_push(n.h_packed, (size_t)32 * c0);
    for (int co = 0; co < c0; ++co)
        for (int k = 0; k < 32; ++k)
            n.h_packed[st.st_w2 + (size_t)k * c0 + co] = rnd((float)((double)w2.data[(size_t)co * 32 + k] * sc[co]));
    st.st_b2 = push_bias(n, sh);
}

// element (co, ci, tap) of conv weights [Cout][Ci][taps] of one or two channel-concatenated sources: the BN scale is
// folded in fp64 before the one rounding to fp32; zero beyond Cout / the channel total
struct Concat {
    std::vector<const Tensor*> ws;
    const std::vector<double>* scale;
    int Cout, Ct = 0, taps;
    Concat(std::vector<const Tensor*> w, const std::vector<double>* s) : ws(std::move(w)), scale(s) {
        Cout = (int)ws[0]->shape[0];
        taps = (int)(ws[0]->shape[2] * ws[0]->shape[3]);
        for (auto* t : ws) Ct += (int)t->shape[1];
    }
    float operator()(int co, int ci, int tap = 0) const {
        if (co >= Cout || ci >= Ct) return 0.f;
        for (auto* w : ws) {
            const int c = (int)w->shape[1];
            if (ci < c) {
                double x = w->data[((size_t)co * c + ci) * taps + tap];
                if (scale) x *= (*scale)[co];
                return (float)x;
            }
            ci -= c;
        }
        return 0.f;
    }
};

// ---------------------------------------------------------------------------------------------------
// fp32 packers
// ---------------------------------------------------------------------------------------------------

// conv [Cout][Cin/g][k][k] + BN -> flat [Cout][rest] scaled, bias
void pack_conv_bn(Net& n, const std::string& wkey, const std::string& bnkey, Op& op) {
    const Tensor& w = T(n, wkey);
    std::vector<double> sc, sh;
    bn_fold(n, op, bnkey, sc, sh);
    const int64_t co = w.shape[0], rest = w.numel() / co;
    op.w_off = arena_push(n.h_packed, (size_t)w.numel());
    for (int64_t o = 0; o < co; ++o)
        for (int64_t r = 0; r < rest; ++r)
            n.h_packed[op.w_off + o * rest + r] = (float)((double)w.data[o * rest + r] * sc[o]);
    op.b_off = push_bias(n, sh);
}

// pointwise weights (optionally two sources) -> fp32 MFMA A fragments [cblocks][K/2][64]; for one source with K a
// multiple of 16 also their exact bf16x3 split (pw3_kernel); bias in D-fragment order
void pack_pw(Net& n, std::vector<const Tensor*> ws, const std::vector<double>* scale, const std::vector<double>* shift,
             Op& op) {
    const Concat w(std::move(ws), scale);
    const int K = w.Ct, cblocks = (w.Cout + 31) / 32;
    // k-pairs per SOURCE (pw2_kernel walks one source at a time): an odd channel count ends in a pair whose second
    // weight is zero, so that no pair straddles the two sources.  Even counts: the plain [K/2] pairs
    const int Ka = (int)w.ws[0]->shape[1], PA = (Ka + 1) / 2, PB = (K - Ka + 1) / 2;
    op.w_off = push_afrag32(n, cblocks, PA + PB, [&](int cb, int row, int k) {
        if (k < 2 * PA) return k < Ka ? w(cb * 32 + row, k) : 0.f;
        return k - 2 * PA < K - Ka ? w(cb * 32 + row, Ka + k - 2 * PA) : 0.f;
    });
    op.ws_off = 0;
    if (w.ws.size() == 1 && (K % 16) == 0) op.ws_off = push_afrag3(n, cblocks, K / 16, w);
    op.has_bias = true;
    op.b_off = push_bias_dfrag(n, cblocks, w.Cout, shift);
}

// depthwise weights with every tap twice, [C][k*k][2] (launch_dw: dw_kernel / dw_pair_kernel / dw_pair16_kernel).  Why:
// these kernels multiply a PAIR of pixels (or of images) by one wave-uniform tap per packed FMA; from the plain [C][k*k]
// array hipcc broadcasts the tap of an odd SGPR with op_sel:[0,1,0] -- the one packed fp32 form that is not safe next to
// bf16 MFMA waves on gfx950 (tools/ubench/pk_vs_mfma.hip).  An aligned (w, w) pair needs no op_sel at all.
void pack_dw_dup(Net& n, Op& op) {
    const size_t cnt = (size_t)op.Ca * op.K * op.K;
    op.wdup_off = arena_push(n.h_packed, 2 * cnt);
    for (size_t i = 0; i < cnt; ++i)
        n.h_packed[op.wdup_off + 2 * i] = n.h_packed[op.wdup_off + 2 * i + 1] = n.h_packed[op.w_off + i];
}

// head depthwise (5x5) for headfuse_kernel: taps + bias of a channel pair interleaved, [C/2][K*K + 1][2]
void pack_head_pairs(Net& n, Op& op) {
    const int C = op.Ca, KK = op.K * op.K;
    if (C & 1) return;
    op.wpair_off = arena_push(n.h_packed, (size_t)(C / 2) * (KK + 1) * 2);
    for (int c = 0; c < C; ++c) {
        for (int k = 0; k < KK; ++k)
            n.h_packed[op.wpair_off + ((size_t)(c >> 1) * (KK + 1) + k) * 2 + (c & 1)] =
                n.h_packed[op.w_off + (size_t)c * KK + k];
        n.h_packed[op.wpair_off + ((size_t)(c >> 1) * (KK + 1) + KK) * 2 + (c & 1)] = n.h_packed[op.b_off + c];
    }
}

// dense conv weights (one or two channel-concatenated sources, [Cout][Ci][K][K] each) -> exact bf16x3 A fragments for
// convk3_kernel: [cblock][tap ky*K+kx][ks][piece][64 lanes][4 dwords], ci = ks*16 + ...; bias [Cout] = shift (+ the
// convs' own biases)
void pack_convk(Net& n, std::vector<const Tensor*> ws, const std::vector<double>* scale, const std::vector<double>& shift,
                Op& op) {
    const Concat w(std::move(ws), scale);
    const int KS = (w.Ct + 15) / 16;
    op.wk_off = push_afrag3(n, (w.Cout + 31) / 32, w.taps * KS, [&](int co, int k) {
        const int step = k >> 4;
        return w(co, (step % KS) * 16 + (k & 15), step / KS);
    });
    op.b_off = push_bias(n, shift);
}

// transposed-conv pair (refined channels, then the raw ones; ww = nullptr for a plain head) with the BN scale folded:
//   w_off / b_off    [ci][co][ky][kx] and the shift: deconv_pair_kernel, and the source of the forms below
//   w2_off / b2_off  Cout <= 32: fp32 MFMA fragments per output parity, k-pairs [tap][refined pairs, raw pairs] (o.mid = 1)
//   w3_off / b3_off  Cout <= 64, even channel counts: one 16-byte fetch = the 4 taps of (channel block, parity, channel
//                    pair, lane); bias in D-fragment order per channel block
//   w4_off           ... and channel counts in eights: exact bf16x3 A fragments [channel block][parity][tap][ks]
void pack_deconv(Net& n, const Tensor& wr, const Tensor* ww, const std::vector<double>& sc, const std::vector<double>& sh,
                 const Deconv& dc, Op& o) {
    const int Ca = dc.refined_in, Ct = Ca + dc.raw_in, Cout = dc.out;
    o.w_off = arena_push(n.h_packed, (size_t)Ct * Cout * 16);
    for (int ci = 0; ci < Ct; ++ci)
        for (int co = 0; co < Cout; ++co)
            for (int t = 0; t < 16; ++t) {
                const double x = ci < Ca ? wr.data[((size_t)ci * Cout + co) * 16 + t]
                                         : ww->data[((size_t)(ci - Ca) * Cout + co) * 16 + t];
                n.h_packed[o.w_off + ((size_t)ci * Cout + co) * 16 + t] = (float)(x * sc[co]);
            }
    o.b_off = push_bias(n, sh);
    // the folded weight of (ci, co) at tap t of parity par, read back by OFFSET: every push below may move the arena
    const size_t w_off = o.w_off;
    auto folded = [&n, w_off, Ct, Cout](int ci, int co, int par, int t) -> float {
        if (ci >= Ct || co >= Cout) return 0.f;
        return n.h_packed[w_off + ((size_t)ci * Cout + co) * 16 + deconv_tap(par, t)];
    };
    if (Cout <= 32) {
        // per tap the refined k-pairs, then the raw ones; an odd source ends in a pair with a zero second weight
        const int Cb = dc.raw_in, PA = (Ca + 1) / 2, PT = PA + (Cb + 1) / 2;
        o.w2_off = push_afrag32(n, 4, 4 * PT, [&](int par, int co, int k) {
            const int t = k / (2 * PT), r = k % (2 * PT);
            if (r < 2 * PA) return r < Ca ? folded(r, co, par, t) : 0.f;
            return r - 2 * PA < Cb ? folded(Ca + r - 2 * PA, co, par, t) : 0.f;
        });
        o.b2_off = push_bias_dfrag(n, 1, Cout, &sh);
        o.mid = 1;                       // flag: MFMA form available
    }
    const int nb = (Cout + 31) / 32;
    if (nb > 2 || (dc.refined_in & 1) || (dc.raw_in & 1) || (Ct & 3)) return;
    const int CP = Ct / 2;
    o.w3_off = arena_push(n.h_packed, (size_t)nb * 4 * CP * 64 * 4);
    for (int cb = 0; cb < nb; ++cb)
        for (int par = 0; par < 4; ++par)
            for (int cp = 0; cp < CP; ++cp)
                for (int l = 0; l < 64; ++l)
                    for (int t = 0; t < 4; ++t)
                        n.h_packed[o.w3_off + ((((size_t)cb * 4 + par) * CP + cp) * 64 + l) * 4 + t] =
                            folded(2 * cp + (l >> 5), cb * 32 + (l & 31), par, t);
    if ((dc.refined_in & 7) == 0 && (dc.raw_in & 7) == 0) {
        const int KS = (Ct + 15) / 16;
        o.w4_off = push_afrag3(n, nb, 16 * KS, [&](int co, int k) {
            const int step = k >> 4, pt = step / KS;          // pt = parity*4 + tap
            return folded((step % KS) * 16 + (k & 15), co, pt >> 2, pt & 3);
        });
    }
    o.b3_off = push_bias_dfrag(n, nb, Cout, &sh);
}

// ---------------------------------------------------------------------------------------------------
// 16-bit storage (bf16 or fp16): folded weights are rounded to the storage format (round-to-nearest-even,
// like v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 and torch's .to(bfloat16) / .to(float16)); biases stay fp32.
// oracle/net_ref.py:forward_bf16 restates the bf16 numerics, tests/_f16_ref.py the fp16 ones.
// ---------------------------------------------------------------------------------------------------

// conv [Cout][rest] + BN -> fp32 values rounded to the storage format; octet = true: depthwise weights as [C/8][rest][8]
void pack_conv_bn_b(Net& n, const std::string& wkey, const std::string& bnkey, BOp& op, bool octet) {
    const Tensor& w = T(n, wkey);
    std::vector<double> sc, sh;
    bn_fold(n, op, bnkey, sc, sh);
    const int64_t co = w.shape[0], rest = w.numel() / co;
    if (octet) {            // [C/8][rest + 1][8]: the octet's taps, then its bias (one LDS-staged block per octet)
        // whole octets only: a channel count that is no multiple of 8 (deconv filters of 20, say) has no 16-bit kernel --
        // every launcher refuses it at the forward, by the layer's name -- and its last channels have no place here
        op.w_off = arena_push(n.h_packed, (size_t)(co / 8) * (rest + 1) * 8);
        for (int64_t o = 0; o < co / 8 * 8; ++o) {
            for (int64_t r = 0; r < rest; ++r)
                n.h_packed[op.w_off + (size_t)((o >> 3) * (rest + 1) + r) * 8 + (o & 7)] =
                    round16(n.storage, (float)((double)w.data[o * rest + r] * sc[o]));
            n.h_packed[op.w_off + (size_t)((o >> 3) * (rest + 1) + rest) * 8 + (o & 7)] = (float)sh[o];
        }
        return;
    }
    op.w_off = arena_push(n.h_packed, (size_t)w.numel());
    for (int64_t o = 0; o < co; ++o)
        for (int64_t r = 0; r < rest; ++r)
            n.h_packed[op.w_off + (size_t)(o * rest + r)] = round16(n.storage, (float)((double)w.data[o * rest + r] * sc[o]));
    op.b_off = push_bias(n, sh);
}

// depthwise KxK (7, 5) taps of an octet-packed op -> banded B fragments of v_mfma_f32_16x16x32_bf16 for dwt_kernel:
// [C][K filter rows][64 lanes][4 dwords]; lane l holds output column n = l & 15 and tile columns
// j = 8 (l >> 4) + 0..7: T[j][n] = w[ky][j - n] for 0 <= j - n < K, else 0 (two bf16 per dword, even j low)
void pack_dwt(Net& n, BOp& op) {
    const int C = op.Ca, K = op.K, KK1 = K * K + 1;
    op.wt_off = arena_push(n.h_packed, (size_t)C * K * 64 * 4);
    uint32_t* d = reinterpret_cast<uint32_t*>(n.h_packed.data() + op.wt_off);
    auto tap = [&](int c, int ky, int kx) -> uint32_t {
        if (kx < 0 || kx >= K) return 0u;
        return (uint32_t)rne16(n, n.h_packed[op.w_off + (size_t)((c >> 3) * KK1 + ky * K + kx) * 8 + (c & 7)]);
    };
    for (int c = 0; c < C; ++c)
        for (int ky = 0; ky < K; ++ky)
            for (int l = 0; l < 64; ++l)
                for (int dq = 0; dq < 4; ++dq) {
                    const int nn = l & 15, j = 8 * (l >> 4) + 2 * dq;
                    d[(((size_t)c * K + ky) * 64 + l) * 4 + dq] = tap(c, ky, j - nn) | (tap(c, ky, j + 1 - nn) << 16);
                }
}

// depthwise 7x7 taps of an octet-packed op -> mbtd_kernel's dot2 operands: per 32-channel chunk 448 records of 16 bytes
// [16 pairs][7 filter rows][channel A even set, A odd set, B even set, B odd set]; behind the last chunk the biases
// [chunk][32 fp32].  A dword = two bf16 taps for the cells of an ALIGNED pair (low half = the even cell): an output at an
// even column takes (w0,w1)(w2,w3)(w4,w5)(w6,0) on the four pairs from its own, one at an odd column (0,w0)(w1,w2)(w3,w4)
// (w5,w6) on the four pairs from the one it sits in.  Channels beyond C (a half chunk) are zero.
void pack_wrow_d(Net& n, BOp& op) {
    const int C = op.Ca, nch = (C + 31) / 32;
    op.wrow2_off = arena_push(n.h_packed, (size_t)nch * (448 * 4 + 32));
    uint32_t* d = reinterpret_cast<uint32_t*>(n.h_packed.data() + op.wrow2_off);
    float* bias = n.h_packed.data() + op.wrow2_off + (size_t)nch * 448 * 4;
    for (int c = 0; c < C; ++c) {
        const size_t src = op.w_off + (size_t)(c >> 3) * 50 * 8 + (c & 7);
        const int chunk = c >> 5, kp = (c & 31) >> 1, ab = c & 1;
        auto tap = [&](int ky, int kx) -> uint32_t {
            if (kx < 0 || kx > 6) return 0u;
            return (uint32_t)rne16(n, n.h_packed[src + (size_t)(ky * 7 + kx) * 8]);
        };
        for (int ky = 0; ky < 7; ++ky) {
            uint32_t* r = d + ((size_t)chunk * 448 + kp * 28 + ky * 4 + 2 * ab) * 4;
            for (int t = 0; t < 4; ++t) {
                r[t] = tap(ky, 2 * t) | (tap(ky, 2 * t + 1) << 16);           // even set
                r[4 + t] = tap(ky, 2 * t - 1) | (tap(ky, 2 * t) << 16);       // odd set
            }
        }
        bias[(size_t)chunk * 32 + (c & 31)] = n.h_packed[src + (size_t)49 * 8];
    }
}

// 1x1 weights (one or two channel-concatenated sources) -> 16-bit A fragments [cblock][ks] + bias in D-fragment order
void pack_pwb(Net& n, std::vector<const Tensor*> ws, const std::vector<double>* scale, const std::vector<double>* shift,
              BOp& op) {
    const Concat w(std::move(ws), scale);
    const int cblocks = (w.Cout + 31) / 32;
    op.w_off = push_afrag16(n, cblocks, (w.Ct + 15) / 16, w);
    op.b_off = push_bias_dfrag(n, cblocks, w.Cout, shift);
}

// deconv pair -> [channel block][parity][tap][ks] 16-bit A fragments (k over the refined channels, then the raw ones;
// BN scale folded into both halves) + the BN shift as bias in D-fragment order.  ww = nullptr (plain head): the
// refined channels only
void pack_deconvb(Net& n, const Tensor& wr, const Tensor* ww, const std::vector<double>& sc, const std::vector<double>& sh,
                  const Deconv& dc, BOp& op) {
    const int Ca = dc.refined_in, Ct = Ca + dc.raw_in, Cout = dc.out, KS = (Ct + 15) / 16, nb = (Cout + 31) / 32;
    op.w_off = push_afrag16(n, nb, 16 * KS, [&](int co, int k) -> float {
        const int step = k >> 4, pt = step / KS, ci = (step % KS) * 16 + (k & 15);   // pt = parity*4 + tap
        if (ci >= Ct || co >= Cout) return 0.f;
        const int tap = deconv_tap(pt >> 2, pt & 3);
        const double x = ci < Ca ? wr.data[((size_t)ci * Cout + co) * 16 + tap]
                                 : ww->data[((size_t)(ci - Ca) * Cout + co) * 16 + tap];
        return (float)(x * sc[co]);
    });
    op.b_off = push_bias_dfrag(n, nb, Cout, &sh);
}

// ---------------------------------------------------------------------------------------------------
// The walk and its sites
// ---------------------------------------------------------------------------------------------------

template <class O>
O make_op(OpType type, const std::string& name, int inA, int out, int Ca, int Cout, int K, int S, int in_div,
          int out_div, int act) {
    O o;
    o.type = type; o.name = name; o.inA = inA; o.out = out; o.Ca = Ca; o.Cout = Cout; o.K = K; o.S = S;
    o.in_div = in_div; o.out_div = out_div; o.act = act;
    return o;
}

// what the walk hands an emitter.  Buffers are ids into n.bufs; a div is the plane's divisor of the input size
struct BlockSite {
    const Block& blk;
    std::string pfx;                       // "stage.S.B": the block's tap, and the prefix of its ops and weights
    int in, div, odiv;
};
struct DeconvSite {
    const Deconv& dc;
    std::string si, name;                  // "I", "deconv.I" (op name and tap)
    int refined, raw, rdiv, raw_div, odiv; // raw = -1, raw_div = 0: plain head
    // the op all forms share: two sources -> dc.out channels at twice the resolution, ReLU
    template <class O>
    O op(OpType type, int K, int out) const {
        O o = make_op<O>(type, name, refined, out, dc.refined_in, dc.out, K, 1, rdiv, odiv, ACT_RELU);
        o.inB = raw;
        o.Cb = dc.raw_in;
        o.tap = name;
        return o;
    }
};
struct HeadSite {
    const Head& h;
    std::string hi;                        // "I" of final_refined.I / final_raw.I / final.I
    int refined, raw, rdiv, raw_div;
    // a head's 5x5 depthwise + BN + ReLU on one source (family 0)
    template <class O>
    O dw(const std::string& branch, int in, int out, int C) const {
        return make_op<O>(OP_DW, branch + hi + ".dw5", in, out, C, C, 5, 1, rdiv, rdiv, ACT_RELU);
    }
};

struct Form {
    Net& n;
    explicit Form(Net& net) : n(net) {}
    virtual ~Form() {}
    virtual int stem() = 0;                                      // -> the buffer of c0 channels at 1/2
    virtual int block(const BlockSite& s) = 0;                   // -> the block's output buffer
    virtual int deconv(const DeconvSite& s, int* out) = 0;       // LP_* code; *out: the deconv's output buffer
    virtual int head(const HeadSite& s, int* out) = 0;           // LP_* code; *out: the head's output buffer
};

int walk(Net& n, Form& f) {
    n.ops.clear();
    n.bops.clear();
    n.bufs = BufferPlan();
    n.h_packed.clear();
    n.out0_buf = n.out1_buf = -1;
    int cur = f.stem(), div = 2;
    std::vector<int> xlist = {cur}, xdiv = {div};
    for (size_t s = 0; s < n.stages.size(); ++s) {
        for (size_t b = 0; b < n.stages[s].size(); ++b) {
            const Block& blk = n.stages[s][b];
            const BlockSite site{blk, "stage." + std::to_string(s) + "." + std::to_string(b), cur, div, div * blk.stride};
            cur = f.block(site);
            div = site.odiv;
        }
        xlist.push_back(cur);
        xdiv.push_back(div);
    }
    // fusion deconv head: deconv i reads the refined tensor and x_list[-i-2], head i-1 the deconv's output and
    // x_list[-i-3] (plain_head: the refined branch only, pose_simplenet.py:128-136)
    const bool plain = n.arch.plain_head == 1;
    const int L = (int)xlist.size();
    int refined = xlist.back(), rdiv = xdiv.back();
    int raw = plain ? -1 : xlist[L - 2], raw_div = plain ? 0 : xdiv[L - 2];
    for (size_t i = 0; i < n.deconv.size(); ++i) {
        const std::string si = std::to_string(i);
        const DeconvSite ds{n.deconv[i], si, "deconv." + si, refined, raw, rdiv, raw_div, rdiv / 2};
        if (const int rc = f.deconv(ds, &refined)) return rc;
        rdiv = ds.odiv;
        if (!plain) {
            const int ri = L - (int)i - 3;
            if (ri < 0) return fail(LP_ERR_UNSUPPORTED, "more deconv layers than backbone taps");
            raw = xlist[ri];
            raw_div = xdiv[ri];
        }
        if (i > 0) {
            const HeadSite hs{n.heads[i - 1], std::to_string(i - 1), refined, raw, rdiv, raw_div};
            if (const int rc = f.head(hs, i == 1 ? &n.out0_buf : &n.out1_buf)) return rc;
        }
    }
    if (n.deconv.size() != 3 || n.out0_buf < 0 || n.out1_buf < 0)
        return fail(LP_ERR_UNSUPPORTED, "the path is built for NUM_DECONV_LAYERS == 3 (two output stages)");
    return LP_OK;
}

// ---------------------------------------------------------------------------------------------------
// Family 0 (pose_mobilenet / pose_simplenet): stem conv3x3 s2 / dw3 / 1x1, InvBottleneck blocks, transposed-conv
// deconvs, heads of dw5 (+ dw5) + 1x1.  P = F32 or B16: the op type, the packers and the block emitter
// ---------------------------------------------------------------------------------------------------
template <class P>
struct Family0 : Form {
    typedef typename P::O O;
    using Form::Form;
    int stem() override {
        const int bStem0 = new_buf(n, 32, 2), bStem1 = new_buf(n, 32, 2), cur = new_buf(n, n.c0, 2);
        O o = make_op<O>(OP_STEM, "stem.conv3x3s2", -1, bStem0, 0, 32, 0, 1, 1, 2, ACT_RELU6);
        P::conv(n, "first.0.0.weight", "first.0.1", o);
        O d = make_op<O>(OP_DW, "stem.dw3", bStem0, bStem1, 32, 32, 3, 1, 2, 2, ACT_RELU6);
        P::dw(n, "first.1.0.weight", "first.1.1", d, false);
        O p = make_op<O>(OP_PW, "stem.pw", bStem1, cur, 32, n.c0, 0, 1, 2, 2, ACT_NONE);
        p.tap = "first";
        std::vector<double> sc, sh;
        bn_fold(n, p, "first.3", sc, sh);
        P::pw(n, {&T(n, "first.2.weight")}, &sc, &sh, p);
        P::fused_stem(n, o, d, sc, sh);
        P::ops(n).insert(P::ops(n).end(), {o, d, p});
        return cur;
    }
    int block(const BlockSite& s) override { return P::block(n, s); }
    int deconv(const DeconvSite& s, int* out) override {
        if (const int rc = P::admit(n, s.dc)) return rc;
        *out = new_buf(n, s.dc.out, s.odiv);
        O o = s.template op<O>(OP_DECONV, 0, *out);
        std::vector<double> sc, sh;
        bn_fold(n, o, "deconv_bnrelu." + s.si + ".0", sc, sh);
        // the packed forms hold the refined channels, then the raw ones (none for a plain head)
        P::deconv(n, T(n, "deconv_refined." + s.si + ".weight"),
                  s.raw < 0 ? nullptr : &T(n, "deconv_raw." + s.si + ".weight"), sc, sh, s.dc, o);
        P::ops(n).push_back(o);
        return LP_OK;
    }
    // one SepConv per source and output stage: dw5 + BN + ReLU, then ONE 1x1 over the concatenated channels
    int head(const HeadSite& s, int* out) override {
        const bool plain = s.raw < 0;
        const int bA = new_buf(n, s.h.refined_in, s.rdiv), bB = plain ? -1 : new_buf(n, s.h.raw_in, s.rdiv);
        *out = new_buf(n, s.h.oup, s.rdiv);
        std::vector<const Tensor*> ws;
        for (int which = 0; which < (plain ? 1 : 2); ++which) {
            const std::string branch = which == 0 ? "final_refined." : "final_raw.";
            O a = which == 0 ? s.template dw<O>(branch, s.refined, bA, s.h.refined_in)
                             : s.template dw<O>(branch, s.raw, bB, s.h.raw_in);
            P::dw(n, branch + s.hi + ".conv.0.weight", branch + s.hi + ".conv.1", a, true);
            P::ops(n).push_back(a);
            ws.push_back(&T(n, branch + s.hi + ".conv.3.weight"));
        }
        O p = make_op<O>(OP_PW, "final." + s.hi + ".pw", bA, *out, s.h.refined_in, s.h.oup, 0, 1, s.rdiv, s.rdiv, ACT_NONE);
        p.inB = bB;
        p.Cb = s.h.raw_in;
        P::pw(n, ws, nullptr, nullptr, p);
        P::head_pw(p, plain);
        P::ops(n).push_back(p);
        return LP_OK;
    }
};

struct F32 {
    typedef Op O;
    static std::vector<Op>& ops(Net& n) { return n.ops; }
    static int admit(Net&, const Deconv&) { return LP_OK; }
    static void conv(Net& n, const std::string& wkey, const std::string& bnkey, Op& o) { pack_conv_bn(n, wkey, bnkey, o); }
    static void dw(Net& n, const std::string& wkey, const std::string& bnkey, Op& o, bool head) {
        pack_conv_bn(n, wkey, bnkey, o);
        if (head) pack_head_pairs(n, o);
        pack_dw_dup(n, o);
    }
    static void pw(Net& n, std::vector<const Tensor*> ws, const std::vector<double>* sc, const std::vector<double>* sh, Op& o) {
        pack_pw(n, std::move(ws), sc, sh, o);
    }
    static void fused_stem(Net& n, Op& st, const Op& dw, const std::vector<double>& sc, const std::vector<double>& sh) {
        pack_fused_stem(n, st, [&](int c, int t) { return dw.w_off + c * 9 + t; }, false, sc, sh, [](float x) { return x; });
    }
    // the one-source head's 1x1 keeps the fp32-MFMA form (no bf16x3 split), the arithmetic of the one-source
    // headfuse_kernel, so that the fused and the unfused head agree bitwise
    static void head_pw(Op& p, bool plain) { if (plain) p.ws_off = 0; }
    static void deconv(Net& n, const Tensor& wr, const Tensor* ww, const std::vector<double>& sc,
                       const std::vector<double>& sh, const Deconv& dc, Op& o) {
        pack_deconv(n, wr, ww, sc, sh, dc, o);
    }
    // expand, then depthwise + project as ONE fused launch (dwpw_kernel); the plan keeps what the unfused fallback needs
    // (shapes the fused kernel does not cover)
    static int block(Net& n, const BlockSite& s) {
        const Block& blk = s.blk;
        const int bE = new_buf(n, blk.feat, s.div), bD = new_buf(n, blk.feat, s.odiv), bO = new_buf(n, blk.oup, s.odiv);
        std::vector<double> sc, sh;
        Op e = make_op<Op>(OP_PW, s.pfx + ".inv", s.in, bE, blk.inp, blk.feat, 0, 1, s.div, s.div, ACT_RELU6);
        bn_fold(n, e, s.pfx + ".inv.1", sc, sh);
        pack_pw(n, {&T(n, s.pfx + ".inv.0.weight")}, &sc, &sh, e);
        e.fuse_next = true;
        n.ops.push_back(e);
        Op d = make_op<Op>(OP_DWPW, s.pfx + ".depth_conv+point_conv", bE, bO, blk.feat, blk.oup, blk.k, blk.stride, s.div,
                           s.odiv, ACT_NONE);
        d.mid = bD;
        d.res = blk.residual ? s.in : -1;
        d.tap = s.pfx;
        dw(n, s.pfx + ".depth_conv.0.weight", s.pfx + ".depth_conv.1", d, false);
        if (blk.k == 7 && (blk.feat & 1) == 0) {
            // the fused block kernels run a channel pair per packed FMA: weights as (w_c[k], w_c+1[k]) pairs
            d.wpair_off = arena_push(n.h_packed, (size_t)blk.feat * 49);
            for (int c = 0; c < blk.feat; ++c)
                for (int k = 0; k < 49; ++k)
                    n.h_packed[d.wpair_off + ((size_t)(c >> 1) * 49 + k) * 2 + (c & 1)] = n.h_packed[d.w_off + (size_t)c * 49 + k];
            d.wrow_off = push_pair_rows(n, blk.feat / 2, blk.feat,
                                        [&](int c, int t) { return t < 49 ? d.w_off + (size_t)c * 49 + t : d.b_off + c; });
        }
        {
            Op p;                           // the project's fragments and bias live in the fused op
            bn_fold(n, d, s.pfx + ".point_conv.1", sc, sh);
            pack_pw(n, {&T(n, s.pfx + ".point_conv.0.weight")}, &sc, &sh, p);
            d.w2_off = p.w_off;
            d.b2_off = p.b_off;
            d.ws_off = p.ws_off;
        }
        n.ops.push_back(d);
        return bO;
    }
};

// every InvBottleneck as expand / depthwise / project (the launch sequence fuses them again where a kernel exists)
struct B16 {
    typedef BOp O;
    static std::vector<BOp>& ops(Net& n) { return n.bops; }
    static int admit(Net& n, const Deconv& dc) {
        if (dc.out > 64) return fail(LP_ERR_UNSUPPORTED, std::string(storage_name(n)) + " storage: deconv filters > 64 are not supported");
        return LP_OK;
    }
    static void conv(Net& n, const std::string& wkey, const std::string& bnkey, BOp& o) { pack_conv_bn_b(n, wkey, bnkey, o, false); }
    static void dw(Net& n, const std::string& wkey, const std::string& bnkey, BOp& o, bool head) {
        pack_conv_bn_b(n, wkey, bnkey, o, true);
        if (head) pack_dwt(n, o);
    }
    static void pw(Net& n, std::vector<const Tensor*> ws, const std::vector<double>* sc, const std::vector<double>* sh, BOp& o) {
        pack_pwb(n, std::move(ws), sc, sh, o);
    }
    // stem4_kernel<Bf16 | F16, C0> exists for c0 = 16 and 24: the SAME rounded folded weights in the fp32 stem's layouts
    static void fused_stem(Net& n, BOp& st, const BOp& dw, const std::vector<double>& sc, const std::vector<double>& sh) {
        if (n.c0 != 16 && n.c0 != 24) return;
        pack_fused_stem(n, st, [&](int c, int t) { return dw.w_off + (size_t)((c >> 3) * 10 + t) * 8 + (c & 7); }, true, sc, sh,
                        [&](float x) { return round16(n.storage, x); });
    }
    static void head_pw(BOp& p, bool) { p.out_f32 = true; }
    static void deconv(Net& n, const Tensor& wr, const Tensor* ww, const std::vector<double>& sc,
                       const std::vector<double>& sh, const Deconv& dc, BOp& o) {
        pack_deconvb(n, wr, ww, sc, sh, dc, o);
    }
    static int block(Net& n, const BlockSite& s) {
        const Block& blk = s.blk;
        const int bE = new_buf(n, blk.feat, s.div), bD = new_buf(n, blk.feat, s.odiv), bO = new_buf(n, blk.oup, s.odiv);
        std::vector<double> sc, sh;
        BOp e = make_op<BOp>(OP_PW, s.pfx + ".inv", s.in, bE, blk.inp, blk.feat, 0, 1, s.div, s.div, ACT_RELU6);
        bn_fold(n, e, s.pfx + ".inv.1", sc, sh);
        pack_pwb(n, {&T(n, s.pfx + ".inv.0.weight")}, &sc, &sh, e);
        BOp d = make_op<BOp>(OP_DW, s.pfx + ".depth_conv", bE, bD, blk.feat, blk.feat, blk.k, blk.stride, s.div, s.odiv, ACT_RELU6);
        pack_conv_bn_b(n, s.pfx + ".depth_conv.0.weight", s.pfx + ".depth_conv.1", d, true);
        if (d.K == 7 && d.S == 1) pack_dwt(n, d);
        if (d.K == 7)             // mbtb_kernel's filter rows: the fp32 plan's layout with the rounded taps, whole 32-channel chunks
            d.wrow_off = push_pair_rows(n, 16 * ((d.Ca + 31) / 32), d.Ca,
                                        [&](int c, int t) { return d.w_off + ((size_t)(c >> 3) * 50 + t) * 8 + (c & 7); });
        if (d.K == 7 && d.S == 1) pack_wrow_d(n, d);
        BOp p = make_op<BOp>(OP_PW, s.pfx + ".point_conv", bD, bO, blk.feat, blk.oup, 0, 1, s.odiv, s.odiv, ACT_NONE);
        p.res = blk.residual ? s.in : -1;
        p.tap = s.pfx;
        bn_fold(n, p, s.pfx + ".point_conv.1", sc, sh);
        pack_pwb(n, {&T(n, s.pfx + ".point_conv.0.weight")}, &sc, &sh, p);
        n.bops.insert(n.bops.end(), {e, d, p});
        return bO;
    }
};

// ---------------------------------------------------------------------------------------------------
// Family 1, pose_resnet (lib/models/pose_resnet.py:34-51,112-131): every k x k conv is an OP_CONVK, a FusedMBConv is
// OP_CONVK (+ReLU6) followed by the 1x1 OP_PW with the residual epilogue (layers.py:83-88).  A kernel reads both of
// its sources on one plane, so sources that differ in resolution are refused here
// ---------------------------------------------------------------------------------------------------
struct Resnet : Form {
    using Form::Form;
    void conv_bn(Op& o, const std::string& wkey, const std::string& bnkey) {
        std::vector<double> sc, sh;
        bn_fold(n, o, bnkey, sc, sh);
        pack_convk(n, {&T(n, wkey)}, &sc, sh, o);
    }
    int stem() override {
        const int bStem = new_buf(n, 32, 2), cur = new_buf(n, n.c0, 2);
        Op a = make_op<Op>(OP_CONVK, "first.0", -1, bStem, 3, 32, 7, 2, 1, 2, ACT_RELU6);
        a.image_in = true;
        conv_bn(a, "first.0.0.weight", "first.0.1");
        Op b = make_op<Op>(OP_CONVK, "first.1", bStem, cur, 32, n.c0, 7, 1, 2, 2, ACT_RELU6);
        b.tap = "first";
        conv_bn(b, "first.1.0.weight", "first.1.1");
        n.ops.insert(n.ops.end(), {a, b});
        return cur;
    }
    int block(const BlockSite& s) override {
        const Block& blk = s.blk;
        const int bE = new_buf(n, blk.feat, s.odiv), bO = new_buf(n, blk.oup, s.odiv);
        Op e = make_op<Op>(OP_CONVK, s.pfx + ".inv", s.in, bE, blk.inp, blk.feat, blk.k, blk.stride, s.div, s.odiv, ACT_RELU6);
        conv_bn(e, s.pfx + ".inv.0.weight", s.pfx + ".inv.1");
        Op p = make_op<Op>(OP_PW, s.pfx + ".point_conv", bE, bO, blk.feat, blk.oup, 0, 1, s.odiv, s.odiv, ACT_NONE);
        p.res = blk.residual ? s.in : -1;
        p.tap = s.pfx;
        std::vector<double> sc, sh;
        bn_fold(n, p, s.pfx + ".point_conv.1", sc, sh);
        pack_pw(n, {&T(n, s.pfx + ".point_conv.0.weight")}, &sc, &sh, p);
        n.ops.insert(n.ops.end(), {e, p});
        return bO;
    }
    int deconv(const DeconvSite& s, int* out) override {
        if (s.raw_div != s.rdiv)
            return fail(LP_ERR_UNSUPPORTED, s.name + ": the raw and the refined source differ in resolution");
        *out = new_buf(n, s.dc.out, s.odiv);
        const Tensor &wr = T(n, "deconv_refined." + s.si + ".conv.weight"), &ww = T(n, "deconv_raw." + s.si + ".conv.weight");
        Op o = s.op<Op>(OP_CONVK, (int)wr.shape[2], *out);
        o.ups = 1;
        // the BN follows the SUM of the two UpConvs: its scale goes into both weight sets, its shift is added once
        std::vector<double> sc, sh;
        bn_fold(n, o, "deconv_bnrelu." + s.si + ".0", sc, sh);
        pack_convk(n, {&wr, &ww}, &sc, sh, o);
        n.ops.push_back(o);
        return LP_OK;
    }
    int head(const HeadSite& s, int* out) override {
        if (s.raw_div != s.rdiv) return fail(LP_ERR_UNSUPPORTED, "final." + s.hi + ": sources differ in resolution");
        *out = new_buf(n, s.h.oup, s.rdiv);
        Op f = make_op<Op>(OP_CONVK, "final." + s.hi, s.refined, *out, s.h.refined_in, s.h.oup, 3, 1, s.rdiv, s.rdiv, ACT_NONE);
        f.inB = s.raw;
        f.Cb = s.h.raw_in;
        // two biased convs summed: one launch over the concatenated channels, both biases added (once each)
        const Tensor &br = T(n, "final_refined." + s.hi + ".bias"), &bw = T(n, "final_raw." + s.hi + ".bias");
        std::vector<double> sh((size_t)s.h.oup);
        for (int c = 0; c < s.h.oup; ++c) sh[c] = (double)br.data[c] + (double)bw.data[c];
        pack_convk(n, {&T(n, "final_refined." + s.hi + ".weight"), &T(n, "final_raw." + s.hi + ".weight")}, nullptr, sh, f);
        n.ops.push_back(f);
        return LP_OK;
    }
};

}  // namespace

const char* last_error() { return g_err.c_str(); }

Cost op_cost(const OpBase& o, int esz, bool out_f32, int NB, int H, int W, CostPart part) {
    const int64_t e = esz, nb = NB, Cin = o.Ca + o.Cb, KK = o.K * o.K;
    const int64_t ipx = (int64_t)(H / o.in_div) * (W / o.in_div), opx = (int64_t)(H / o.out_div) * (W / o.out_div);
    Cost c;
    switch (o.type) {
        case OP_STEM:                        // the fp32 image in, 32 channels out
            c.bytes = nb * (12ll * H * W + e * 32 * opx);
            c.flops = c.flops_valu = 2 * nb * 32 * 27 * opx;
            break;
        case OP_PW:                          // in (+ second source) + out (+ residual)
            c.bytes = nb * opx * (e * Cin + (out_f32 ? 4 : e) * o.Cout + (o.res >= 0 ? e * o.Cout : 0));
            c.flops = 2 * nb * opx * Cin * o.Cout;
            break;
        case OP_DECONV:                      // 4 of its 16 taps reach an output cell
        case OP_CONVK:
            c.bytes = e * nb * (Cin * ipx + o.Cout * opx);
            c.flops = 2 * nb * Cin * o.Cout * opx * (o.type == OP_DECONV ? 4 : KK);
            break;
        case OP_DW:
        case OP_DWPW:                        // per reference op: depthwise in + out, then the 1x1's in + out (+ residual)
            if (part != COST_PW_HALF) {
                c.bytes = e * nb * o.Ca * (ipx + opx);
                c.flops = c.flops_valu = 2 * nb * o.Ca * KK * opx;
            }
            if (o.type == OP_DWPW && part != COST_DW_HALF) {
                c.bytes += e * nb * opx * (o.Ca + (int64_t)o.Cout * (o.res >= 0 ? 2 : 1));
                c.flops += 2 * nb * opx * o.Ca * o.Cout;
            }
            break;
    }
    return c;
}

size_t arena_push(std::vector<float>& a, size_t count) {
    // keep every block 64-float (256-byte) aligned
    size_t off = (a.size() + 63) / 64 * 64;
    a.resize(off + count, 0.f);
    return off;
}

float round16(int storage, float x) {
    if (storage == LP_STORAGE_F16) {
        volatile float v = x;
        return (float)(_Float16)v;
    }
    const uint32_t u = (uint32_t)bf16_rne(x) << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

int build(Net& n) {
    if (n.arch.family == 1) {
        if (n.storage != LP_STORAGE_F32)
            return fail(LP_ERR_UNSUPPORTED, "pose_resnet family: fp32 storage only (no 16-bit dense-conv kernels yet)");
        Resnet f(n);
        return walk(n, f);
    }
    if (n.storage != LP_STORAGE_F32) {
        Family0<B16> f(n);
        return walk(n, f);
    }
    Family0<F32> f(n);
    return walk(n, f);
}

int init_arch(Net& n, const lp_arch& arch) {
    const lp_arch* a = &arch;
    if (a->num_stages < 1 || a->num_stages > LP_MAX_STAGES || a->num_deconv != 3)
        return fail(LP_ERR_UNSUPPORTED, "num_stages must be 1..8 and num_deconv 3");
    if (a->plain_head != 0 && a->plain_head != 1) return fail(LP_ERR_INVALID_ARG, "plain_head must be 0 or 1");
    if (a->family != 0 && a->family != 1) return fail(LP_ERR_INVALID_ARG, "family must be 0 or 1");
    const bool resnet = a->family == 1;
    int upk = 3;
    if (resnet) {
        if (a->plain_head) return fail(LP_ERR_INVALID_ARG, "family 1 (pose_resnet) has no plain-head form");
        upk = a->upconv_kernel == 0 ? 3 : a->upconv_kernel;
        if (upk < 0 || (upk & 1) == 0)
            return fail(LP_ERR_INVALID_ARG, "upconv_kernel must be odd (an even kernel does not double the plane)");
        if (upk > 7) return fail(LP_ERR_UNSUPPORTED, "upconv_kernel must be 3, 5 or 7");
    }
    n.arch = *a;
    n.c0 = make_divisible(a->input_channel * 1.0, 8);
    n.channel = {n.c0};
    int inp = n.c0;
    for (int s = 0; s < a->num_stages; ++s) {
        const int c = make_divisible(a->channel[s] * 1.0, 8);
        std::vector<Block> blocks;
        if (a->num_blocks[s] < 1 || a->num_blocks[s] > LP_MAX_BLOCKS) return fail(LP_ERR_INVALID_ARG, "num_blocks out of range");
        for (int b = 0; b < a->num_blocks[s]; ++b) {
            Block blk;
            blk.inp = inp;
            blk.feat = make_divisible(std::nearbyint((double)inp * a->expand[s][b]), 8);
            blk.oup = c;
            blk.k = a->kernel[s][b];
            blk.stride = b == 0 ? a->stride[s] : 1;
            blk.residual = blk.stride == 1 && inp == c;
            if ((blk.k != 3 && blk.k != 5 && blk.k != 7) || (blk.stride != 1 && blk.stride != 2))
                return fail(LP_ERR_UNSUPPORTED, "depthwise kernel must be 3/5/7 and stride 1/2");
            blocks.push_back(blk);
            inp = c;
        }
        n.stages.push_back(blocks);
        n.channel.push_back(c);
    }
    int inplanes = n.channel.back();
    const int L = (int)n.channel.size();
    const bool plain = a->plain_head == 1;      // pose_simplenet.py: no raw branches, so no backbone taps x_list[-i-2/-i-3]
    for (int i = 0; i < a->num_deconv; ++i) {
        if (!plain && L - i - 2 < 0) return fail(LP_ERR_UNSUPPORTED, "too few stages");
        n.deconv.push_back({inplanes, plain ? 0 : n.channel[L - i - 2], a->deconv_filters[i]});
        inplanes = a->deconv_filters[i];
    }
    for (int i = 1; i < a->num_deconv; ++i) {
        if (!plain && L - i - 3 < 0) return fail(LP_ERR_UNSUPPORTED, "too few stages");
        n.heads.push_back({a->deconv_filters[i], plain ? 0 : n.channel[L - i - 3], a->head_channels[i - 1]});
    }
    const std::string conv = resnet ? ".conv.weight" : ".weight";
    if (resnet) {
        // ---- pose_resnet.py:34-60 registration order: first, stage, deconv_refined, deconv_raw, deconv_bnrelu,
        // final_refined, final_raw ----
        add_tensor(n, "first.0.0.weight", {32, 3, 7, 7});
        add_bn(n, "first.0.1", 32);
        add_tensor(n, "first.1.0.weight", {n.c0, 32, 7, 7});
        add_bn(n, "first.1.1", n.c0);
    } else {
        // ---- reference state_dict key scheme, registration order ----
        add_tensor(n, "first.0.0.weight", {32, 3, 3, 3});
        add_bn(n, "first.0.1", 32);
        add_tensor(n, "first.1.0.weight", {32, 1, 3, 3});
        add_bn(n, "first.1.1", 32);
        add_tensor(n, "first.2.weight", {n.c0, 32, 1, 1});
        add_bn(n, "first.3", n.c0);
    }
    for (size_t s = 0; s < n.stages.size(); ++s)
        for (size_t b = 0; b < n.stages[s].size(); ++b) {
            const Block& blk = n.stages[s][b];
            const std::string p = "stage." + std::to_string(s) + "." + std::to_string(b);
            if (resnet) {
                add_tensor(n, p + ".inv.0.weight", {blk.feat, blk.inp, blk.k, blk.k});
                add_bn(n, p + ".inv.1", blk.feat);
            } else {
                add_tensor(n, p + ".inv.0.weight", {blk.feat, blk.inp, 1, 1});
                add_bn(n, p + ".inv.1", blk.feat);
                add_tensor(n, p + ".depth_conv.0.weight", {blk.feat, 1, blk.k, blk.k});
                add_bn(n, p + ".depth_conv.1", blk.feat);
            }
            add_tensor(n, p + ".point_conv.0.weight", {blk.oup, blk.feat, 1, 1});
            add_bn(n, p + ".point_conv.1", blk.oup);
        }
    // UpConv weights are [out][in][k][k], ConvTranspose2d weights [in][out][4][4]
    for (int which = 0; which < (plain ? 1 : 2); ++which)
        for (size_t i = 0; i < n.deconv.size(); ++i) {
            const Deconv& d = n.deconv[i];
            const int cin = which == 0 ? d.refined_in : d.raw_in;
            const std::string key = std::string(which == 0 ? "deconv_refined." : "deconv_raw.") + std::to_string(i) + conv;
            if (resnet) add_tensor(n, key, {d.out, cin, upk, upk});
            else add_tensor(n, key, {cin, d.out, 4, 4});
        }
    for (size_t i = 0; i < n.deconv.size(); ++i) add_bn(n, "deconv_bnrelu." + std::to_string(i) + ".0", n.deconv[i].out);
    for (int which = 0; which < (plain ? 1 : 2); ++which)
        for (size_t i = 0; i < n.heads.size(); ++i) {
            const int cin = which == 0 ? n.heads[i].refined_in : n.heads[i].raw_in;
            const std::string p = std::string(which == 0 ? "final_refined." : "final_raw.") + std::to_string(i);
            if (resnet) {
                add_tensor(n, p + ".weight", {n.heads[i].oup, cin, 3, 3});
                add_tensor(n, p + ".bias", {n.heads[i].oup});
            } else {
                add_tensor(n, p + ".conv.0.weight", {cin, 1, 5, 5});
                add_bn(n, p + ".conv.1", cin);
                add_tensor(n, p + ".conv.3.weight", {n.heads[i].oup, cin, 1, 1});
            }
        }
    return LP_OK;
}

}  // namespace lp_plan
