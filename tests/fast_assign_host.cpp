// Host build of the device's grouping routine (litepose_amd/csrc/fast_assign.h) for tests/test_fast_parse_cpu.py: the same
// text fast_assign_kernel runs per lane, on a plain array of cells.  Built there with the host compiler and
// -ffp-contract=off into a shared object and called through ctypes on the reference's golden peak lists.
#include <cstring>

#include "../litepose_amd/csrc/fast_assign.h"

namespace {
struct HostMem {
    lp::fast::Cell* c;
    lp::fast::Cell& operator[](int w) const { return c[w]; }
};
}  // namespace

// one image: cnt [C], val / tag [C][M], ind [C][M][2], order [C] -> ans [M][C][4]; returns num (-1: round cap)
extern "C" int fast_assign_host(const int* cnt, const float* val, const float* tag, const int* ind, const int* order,
                                int C, int M, float threshold, float* ans) {
    if (C < 1 || C > 32 || M < 1 || M > lp::fast::MAX_PEOPLE) return -2;
    lp::fast::Cell cells[lp::fast::C_WORDS];
    std::memset(cells, 0, sizeof(cells));
    lp::fast::JointOrder jo;
    for (int i = 0; i < 32; ++i) jo.v[i] = i < C ? order[i] : 0;
    std::memset(ans, 0, sizeof(float) * M * C * 4);
    const int num = lp::fast::assign_image(HostMem{cells}, cnt, val, tag, ind, jo, C, M, threshold, ans);
    if (num < 0) std::memset(ans, 0, sizeof(float) * M * C * 4);
    return num;
}
