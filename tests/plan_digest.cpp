// Digests of the network plan (csrc/plan.cpp) for a fixed list of nets: one line per net with three 64-bit FNV-1a
// digests -- the packed weight arena as bytes, the op list field by field, and the buffer plan with the two output
// buffer ids -- or the refusal's message.  tests/test_plan_cpu.py compiles this, runs it and compares the lines with
// tests/golden/plan_digests.txt.  Host code only: no GPU, no Python, no files.
//
//   plan_digest            the digest lines
//   plan_digest --time     milliseconds to build the plan of prune-L in the three storages (minimum of five runs each)
//   plan_digest --costs    lp_plan::op_cost of every op of two plans (search-XS fp32 and bf16, 2 images of 256 x 256)
//
// The golden file was recorded from the engine as it was BEFORE plan.cpp existed: -DPLAN_DIGEST_PARENT='"<engine.cpp>"'
// includes that one-file engine instead of plan.h (its plan builders make no HIP call; linked against that commit's
// library for the launchers it names) and everything below the adaptor is the same code.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef PLAN_DIGEST_PARENT
#include PLAN_DIGEST_PARENT
typedef lp_net Net;
static Net* net_new(const lp_arch& a, std::string& err) {
    lp_net* n = nullptr;
    if (lp_net_create(&n, &a) != LP_OK) { err = lp_last_error(); return nullptr; }
    return n;
}
static void net_free(Net* n) { lp_net_destroy(n); }
static int net_build(Net* n, std::string& err) {
    int rc;
    if (n->arch.family == 1 && n->storage != LP_STORAGE_F32)
        rc = fail(LP_ERR_UNSUPPORTED, "pose_resnet family: fp32 storage only (no 16-bit dense-conv kernels yet)");
    else
        rc = n->arch.family == 1 ? build_plan_resnet(n) : (n->storage != LP_STORAGE_F32 ? build_plan_bf16(n) : build_plan(n));
    if (rc != LP_OK) err = lp_last_error();
    return rc;
}
static void bn_keys(const Op& o, std::string& k0, std::string& k1) { calib_bn_keys(o, k0, k1); }
#else
#include "../litepose_amd/csrc/plan.h"
using namespace lp_plan;
static Net* net_new(const lp_arch& a, std::string& err) {
    Net* n = new Net();
    if (init_arch(*n, a) != LP_OK) { err = last_error(); delete n; return nullptr; }
    return n;
}
static void net_free(Net* n) { delete n; }
static int net_build(Net* n, std::string& err) {
    const int rc = build(*n);
    if (rc != LP_OK) err = last_error();
    return rc;
}
static void bn_keys(const Op& o, std::string& k0, std::string& k1) { k0 = o.bn0; k1 = o.bn1; }
#endif

namespace {

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    }
    void i(int64_t v) { bytes(&v, 8); }
    void s(const std::string& v) { i((int64_t)v.size()); bytes(v.data(), v.size()); }
};

// every tensor from one integer generator: multiples of 1/1024 in [-1, 1]; running_var through abs + 0.5
void fill(Net* n, uint64_t seed) {
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 1;
    for (auto& t : n->tensors) {
        t.is_set = true;
        if (t.is_counter) continue;
        t.data.resize((size_t)t.numel());
        const bool var = t.key.size() > 11 && t.key.compare(t.key.size() - 11, 11, "running_var") == 0;
        for (auto& v : t.data) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            v = (float)((int)((x >> 33) % 2049) - 1024) * (1.0f / 1024.0f);
            if (var) v = (v < 0 ? -v : v) + 0.5f;
        }
    }
}

// the fields Op and BOp share (the 16-bit plan's type values are the fp32 plan's first four)
template <class O>
void common_fields(Fnv& f, const O& o) {
    f.i((int)o.type); f.s(o.name); f.s(o.tap);
    f.i(o.inA); f.i(o.inB); f.i(o.res); f.i(o.out);
    f.i(o.Ca); f.i(o.Cb); f.i(o.Cout); f.i(o.K); f.i(o.S); f.i(o.act);
    f.i(o.in_div); f.i(o.out_div);
    f.i((int64_t)o.w_off); f.i((int64_t)o.b_off);
}

uint64_t ops_digest(const Net* n) {
    Fnv f;
    if (n->storage != LP_STORAGE_F32) {
        f.i((int64_t)n->bops.size());
        for (const BOp& o : n->bops) {
            common_fields(f, o);
            f.i((int64_t)o.wt_off); f.i((int64_t)o.wrow_off); f.i((int64_t)o.wrow2_off); f.i(o.out_f32);
            f.i((int64_t)o.st_w0); f.i((int64_t)o.st_w1); f.i((int64_t)o.st_b1); f.i((int64_t)o.st_w2); f.i((int64_t)o.st_b2);
        }
        return f.h;
    }
    f.i((int64_t)n->ops.size());
    for (const Op& o : n->ops) {
        common_fields(f, o);
        f.i((int64_t)o.w2_off); f.i((int64_t)o.b2_off); f.i((int64_t)o.ws_off); f.i((int64_t)o.wdup_off);
        f.i((int64_t)o.wpair_off); f.i((int64_t)o.w3_off); f.i((int64_t)o.b3_off); f.i((int64_t)o.w4_off);
        f.i((int64_t)o.st_w0); f.i((int64_t)o.st_w1); f.i((int64_t)o.st_w2); f.i((int64_t)o.st_b2);
        f.i((int64_t)o.wrow_off); f.i(o.mid); f.i((int64_t)o.wk_off); f.i(o.ups); f.i(o.image_in); f.i(o.has_bias);
        f.i(o.fuse_next);
        if (n->arch.family == 0) {          // the BatchNorms behind the op: what the calibration layer list is made from
            std::string k0, k1;
            bn_keys(o, k0, k1);
            f.s(k0); f.s(k1);
        }
    }
    return f.h;
}

uint64_t bufs_digest(const Net* n) {
    Fnv f;
    f.i((int64_t)n->bufs.ch.size());
    for (int c : n->bufs.ch) f.i(c);
    for (int d : n->bufs.div) f.i(d);
    f.i(n->out0_buf); f.i(n->out1_buf);
    return f.h;
}

struct Stage { int stride, channel; std::vector<std::pair<int, int>> blocks; };   // blocks: (expand, kernel)

lp_arch make_arch(int family, int input_channel, const std::vector<Stage>& st, const int deconv[3], int plain, int upk) {
    lp_arch a;
    std::memset(&a, 0, sizeof(a));
    a.family = family;
    a.plain_head = plain;
    a.upconv_kernel = upk;
    a.input_channel = input_channel;
    a.num_stages = (int)st.size();
    for (size_t s = 0; s < st.size() && s < LP_MAX_STAGES; ++s) {
        a.num_blocks[s] = (int)st[s].blocks.size();
        a.stride[s] = st[s].stride;
        a.channel[s] = st[s].channel;
        for (size_t b = 0; b < st[s].blocks.size() && b < LP_MAX_BLOCKS; ++b) {
            a.expand[s][b] = st[s].blocks[b].first;
            a.kernel[s][b] = st[s].blocks[b].second;
        }
    }
    a.num_deconv = 3;
    for (int i = 0; i < 3; ++i) a.deconv_filters[i] = deconv[i];
    a.head_channels[0] = 34;                 // 17 joints: heatmaps + tags, then heatmaps alone
    a.head_channels[1] = 17;
    return a;
}

// litepose_amd/arch_zoo.py: the published family-0 nets (6 / 8 / 10 / 10 blocks of [6, 7], strides 2 2 2 1)
struct Zoo { const char* name; int cin; int ch[4]; int deconv[3]; };
const Zoo ZOO[] = {
    {"search-XS", 16, {16, 32, 48, 80}, {16, 24, 24}},  {"search-S", 16, {16, 32, 48, 120}, {32, 24, 32}},
    {"search-M", 16, {24, 48, 72, 120}, {64, 40, 32}},  {"search-L", 24, {24, 64, 96, 160}, {64, 40, 32}},
    {"prune-S", 16, {16, 32, 48, 80}, {32, 24, 16}},    {"prune-M", 24, {24, 48, 72, 120}, {48, 40, 24}},
    {"prune-L", 24, {32, 64, 96, 160}, {64, 48, 32}},
};
lp_arch zoo(const char* name, int plain) {
    for (const Zoo& z : ZOO)
        if (!std::strcmp(z.name, name)) {
            const int nb[4] = {6, 8, 10, 10}, strides[4] = {2, 2, 2, 1};
            std::vector<Stage> st;
            for (int s = 0; s < 4; ++s) st.push_back({strides[s], z.ch[s], std::vector<std::pair<int, int>>(nb[s], {6, 7})});
            return make_arch(0, z.cin, st, z.deconv, plain, 0);
        }
    std::fprintf(stderr, "no zoo net %s\n", name);
    std::exit(2);
}
// c0 = 32; depthwise kernels 3 / 5 / 7 at strides 1 and 2; expanded widths 144, 120, 336 (no multiples of 32)
lp_arch mixed(const int deconv[3], int plain) {
    const std::vector<Stage> st = {
        {2, 24, {{6, 3}, {6, 5}, {6, 7}}},
        {2, 40, {{4, 5}, {3, 7}, {6, 3}}},
        {2, 56, {{6, 7}, {6, 3}, {6, 5}}},
        {1, 88, {{6, 7}, {6, 5}}},
    };
    return make_arch(0, 32, st, deconv, plain, 0);
}
// litepose_amd/models/pose_resnet.py BACKBONE_SETTING with tests/golden/resnet.yaml's deconv widths
lp_arch resnet(int upk, const int strides[4]) {
    const int r = 4, k[4] = {7, 7, 5, 3}, c[4] = {16, 32, 48, 80}, nb[4] = {4, 6, 8, 8}, deconv[3] = {16, 24, 24};
    std::vector<Stage> st;
    for (int s = 0; s < 4; ++s) st.push_back({strides[s], c[s], std::vector<std::pair<int, int>>(nb[s], {r, k[s]})});
    lp_arch a = make_arch(1, 16, st, deconv, 0, upk);
    a.head_channels[0] = 28;                 // 14 joints
    a.head_channels[1] = 14;
    return a;
}

enum Tweak { NONE, IDENTITY_FOLD, DROP_STAGE, DROP_DECONV };
const char* STORAGE_NAME[3] = {"f32", "bf16", "f16"};

void report(const char* name, const lp_arch& a, int storage, Tweak tweak = NONE) {
    std::string err;
    std::printf("%s %s: ", name, STORAGE_NAME[storage]);
    Net* n = net_new(a, err);
    if (!n) { std::printf("refused: %s\n", err.c_str()); return; }
    n->storage = storage;
    if (tweak == IDENTITY_FOLD) n->identity_fold = true;
    if (tweak == DROP_STAGE) n->stages.pop_back();          // what lp_arch cannot say: fewer backbone taps than the head reads
    if (tweak == DROP_DECONV) n->deconv.pop_back();          // ... and a head of two deconvs
    fill(n, 1);
    if (net_build(n, err) != LP_OK) {
        std::printf("refused: %s\n", err.c_str());
    } else {
        Fnv f;
        f.bytes(n->h_packed.data(), n->h_packed.size() * sizeof(float));
        std::printf("packed %016llx (%zu floats) ops %016llx bufs %016llx\n", (unsigned long long)f.h, n->h_packed.size(),
                    (unsigned long long)ops_digest(n), (unsigned long long)bufs_digest(n));
    }
    net_free(n);
}

void time_plans() {
    for (int storage = 0; storage < 3; ++storage) {
        double best = 1e30;
        for (int run = 0; run < 5; ++run) {
            std::string err;
            Net* n = net_new(zoo("prune-L", 0), err);
            n->storage = storage;
            fill(n, 1);
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = net_build(n, err);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc != LP_OK) { std::printf("prune-L refused: %s\n", err.c_str()); std::exit(1); }
            std::printf("prune-L %s run %d: %.2f ms\n", STORAGE_NAME[storage], run, ms);
            if (ms < best) best = ms;
            net_free(n);
        }
        std::printf("prune-L %s min of 5: %.2f ms\n", STORAGE_NAME[storage], best);
    }
}

#ifndef PLAN_DIGEST_PARENT
void print_cost(const OpBase& o, const char* part, const Cost& c) {
    std::printf("%-36s %-4s bytes %lld flops %lld valu %lld\n", o.name.c_str(), part, (long long)c.bytes, (long long)c.flops,
                (long long)c.flops_valu);
}
void costs() {
    for (int storage = 0; storage < 2; ++storage) {
        std::string err;
        Net* n = net_new(zoo("search-XS", 0), err);
        n->storage = storage;
        fill(n, 1);
        if (net_build(n, err) != LP_OK) { std::printf("refused: %s\n", err.c_str()); std::exit(1); }
        for (const Op& o : n->ops) {
            print_cost(o, "op", op_cost(o, 4, false, 2, 256, 256));
            if (o.type != OP_DWPW) continue;
            print_cost(o, "dw", op_cost(o, 4, false, 2, 256, 256, COST_DW_HALF));
            print_cost(o, "pw", op_cost(o, 4, false, 2, 256, 256, COST_PW_HALF));
        }
        for (const BOp& o : n->bops) print_cost(o, "op", op_cost(o, 2, o.out_f32, 2, 256, 256));
        net_free(n);
    }
}
#endif

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--time")) { time_plans(); return 0; }
#ifndef PLAN_DIGEST_PARENT
    if (argc > 1 && !std::strcmp(argv[1], "--costs")) { costs(); return 0; }
#endif
    const int d_wide[3] = {96, 18, 24};      // > 64 (fp32 only); 18: the next deconv has no w3 / w4 form
    const int d_mid[3] = {48, 20, 24};       // 33..64; 20: the next deconv has the w3 form but no w4
    const int s_net[4] = {2, 2, 2, 1}, s_deep[4] = {2, 2, 2, 2}, s_head[4] = {2, 1, 2, 1};
    for (int st = 0; st < 3; ++st) {
        // fusion head: c0 16 / 24 / 32, deconv filters <= 32 and 33..64, head widths 34 and 17
        report("search-XS", zoo("search-XS", 0), st);
        report("prune-M", zoo("prune-M", 0), st);
        report("mixed-48-20-24", mixed(d_mid, 0), st);
        report("mixed-96-18-24", mixed(d_wide, 0), st);       // 16-bit: deconv filters > 64 are refused
        // plain head
        report("search-XS plain", zoo("search-XS", 1), st);
        report("mixed-48-20-24 plain", mixed(d_mid, 1), st);
    }
    report("search-XS identity-fold", zoo("search-XS", 0), 0, IDENTITY_FOLD);
    report("resnet k3", resnet(3, s_net), 0);
    report("resnet k5", resnet(5, s_net), 0);
    // refusals of the plan
    report("resnet k3", resnet(3, s_net), 1);
    report("resnet strides 2 2 2 2", resnet(3, s_deep), 0);
    report("resnet strides 2 1 2 1", resnet(3, s_head), 0);
    report("search-XS less one stage", zoo("search-XS", 0), 0, DROP_STAGE);
    report("search-XS less one deconv", zoo("search-XS", 0), 0, DROP_DECONV);
    // refusals of the architecture
    {
        lp_arch a = zoo("search-XS", 0);
        a.num_deconv = 2;
        report("num_deconv 2", a, 0);
        a = zoo("search-XS", 0);
        a.plain_head = 2;
        report("plain_head 2", a, 0);
        a = zoo("search-XS", 0);
        a.family = 2;
        report("family 2", a, 0);
        a = resnet(3, s_net);
        a.plain_head = 1;
        report("resnet plain", a, 0);
        report("resnet k4", resnet(4, s_net), 0);
        report("resnet k9", resnet(9, s_net), 0);
        a = zoo("search-XS", 0);
        a.num_blocks[1] = 0;
        report("no blocks", a, 0);
        a = zoo("search-XS", 0);
        a.kernel[2][3] = 4;
        report("depthwise 4x4", a, 0);
        a = zoo("search-XS", 0);
        a.num_stages = 3;
        report("three stages", a, 0);
    }
    return 0;
}
