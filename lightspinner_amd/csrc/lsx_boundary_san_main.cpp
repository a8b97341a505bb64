// lsx_boundary_san_main.cpp -- the host-side rules of lsx_hip_set_boundary (lsx_boundary_prep.h) under -fsanitize=address,undefined:
// a stand-alone program (`make bndsan`), nothing is loaded into python.  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "lsx_boundary_prep.h"

using namespace lsxbnd;

static int failed = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failed; } \
    } while (0)

int main()
{
    const int64_t nc = 7;
    const size_t per = 3 * 5;
    std::vector<double> a(nc * per, 1.0);
    const double* A = a.data();
    const int Z = LSX_BOUNDARY_ZERO, T = LSX_BOUNDARY_THERMALISED, G = LSX_BOUNDARY_GIVEN;
    // accepted: every pair of kinds with exactly the arrays it needs
    for (int lo : {Z, T, G})
        for (int up : {Z, T, G}) EXPECT(check_args(nc, 0, nc, lo, up, lo == G ? A : nullptr, up == G ? A : nullptr) == nullptr);
    EXPECT(check_args(nc, 6, 1, T, Z, nullptr, nullptr) == nullptr);
    // refused: unknown kinds, missing and superfluous arrays, ranges
    EXPECT(check_args(nc, 0, 1, 3, Z, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 0, 1, T, -1, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 0, 1, G, Z, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 0, 1, Z, G, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 0, 1, Z, G, A, A) != nullptr);
    EXPECT(check_args(nc, 0, 1, T, Z, A, nullptr) != nullptr);
    EXPECT(check_args(nc, 0, 1, T, Z, nullptr, A) != nullptr);
    EXPECT(check_args(nc, -1, 1, T, Z, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 0, 0, T, Z, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 5, 3, T, Z, nullptr, nullptr) != nullptr);
    EXPECT(check_args(nc, 2147483647LL, 2147483647LL, T, Z, nullptr, nullptr) != nullptr);
    // the kinds' host copy and the store's layout: every (end, column) block inside [2][nc][per], no two alike
    std::vector<int32_t> k(2 * nc, -1);
    default_kinds(k.data(), nc);
    for (int64_t c = 0; c < nc; ++c) EXPECT(k[2 * c] == T && k[2 * c + 1] == Z);
    set_kinds(k.data(), 2, 3, G, T);
    for (int64_t c = 0; c < nc; ++c) {
        const bool in = c >= 2 && c < 5;
        EXPECT(k[2 * c] == (in ? G : T) && k[2 * c + 1] == (in ? T : Z));
    }
    std::vector<int> seen(2 * nc * per, 0);
    for (int end = 0; end < 2; ++end)
        for (int64_t c = 0; c < nc; ++c) {
            const size_t o = store_offset(end, nc, c, per);
            EXPECT(o + per <= seen.size());
            for (size_t e = 0; e < per && o + e < seen.size(); ++e) seen[o + e]++;
        }
    for (int v : seen) EXPECT(v == 1);
    if (!failed) std::printf("ok\n");
    return failed ? 1 : 0;
}
