// host_rows_check.cpp -- stand-alone check of the host-order row movers of crazyflie_nmpc_amd/csrc/cfnmpc_rows.hpp (Layout,
// move_rows, in_place): plain C++, no GPU, no HIP call.  Round-trips int and double columns -- one per stage (fleet stride !=
// row length), one not requested -- through a non-contiguous, unordered index set and checks placement, alignment and that
// nothing outside the rows of the set is written.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_rows_check.cpp -o host_rows_check
//   ./host_rows_check
// (make -C crazyflie_nmpc_amd/csrc host_rows_check; tests/test_host_rows_cpu.py builds and runs it the same way)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../crazyflie_nmpc_amd/csrc/cfnmpc_rows.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int B = 11, N = 5, Nmax = 17;
    const std::vector<int> idx = {7, 0, 8, 4, 10};                         // a bucket's rows in the fleet: unordered, with gaps
    const size_t count = idx.size();
    std::vector<double> yref((size_t)B * Nmax * 3), res(B), unused(B, -1.0);
    std::vector<int> motvel((size_t)B * 3);
    for (size_t i = 0; i < yref.size(); i++) yref[i] = 0.5 + (double)i;
    for (size_t i = 0; i < res.size(); i++) res[i] = -100.0 - (double)i;
    for (size_t i = 0; i < motvel.size(); i++) motvel[i] = 1000 + (int)i;
    const double* none = nullptr;

    // an odd count of ints first, so that the doubles behind it need the padding
    const cfn::Cols cols = {cfn::col(motvel.data(), 3), cfn::col_stages(yref.data(), 3), cfn::col(none, 9), cfn::col(res.data(), 1)};
    const cfn::Layout L(cols, count, N, Nmax);
    CHECK(L.n == 4 && L.len[1] == 15 && L.stride[1] == 51 && L.len[0] == 3 && L.stride[0] == 3);
    CHECK(L.bytes == 64 + count * 15 * 8 + count * 8);                 // 5 x 3 ints + 4 bytes, then the stage rows, nothing for `none`, then res
    std::vector<double> stage(L.bytes / 8 + 1, -7.0);                    // (one guard element behind)
    const cfn::Staged p = cfn::staged(L, stage.data());
    CHECK(p.p[2] == nullptr && p.p[0] == stage.data());
    for (int i = 0; i < 4; i++) CHECK((uintptr_t)p.p[i] % 8 == 0);

    cfn::move_rows<true>(L, stage.data(), idx.data(), count);
    for (size_t r = 0; r < count; r++) {
        for (int e = 0; e < 3; e++) CHECK(p.i(0)[r * 3 + e] == motvel[(size_t)idx[r] * 3 + e]);
        for (int e = 0; e < 15; e++) CHECK(p.d(1)[r * 15 + e] == yref[(size_t)idx[r] * 51 + e]);
        CHECK(p.d(3)[r] == res[idx[r]]);
    }
    CHECK(stage.back() == -7.0);

    // back into prefilled arrays: the rows of the set arrive, the stages behind N and every other vehicle keep the fill
    std::vector<double> yref2(yref.size(), -1.0), res2(B, -1.0);
    std::vector<int> motvel2(motvel.size(), -1);
    const cfn::Cols back = {cfn::col(motvel2.data(), 3), cfn::col_stages(yref2.data(), 3), cfn::col(none, 9), cfn::col(res2.data(), 1)};
    cfn::move_rows<false>(cfn::Layout(back, count, N, Nmax), stage.data(), idx.data(), count);
    for (int v = 0; v < B; v++) {
        bool in = false;
        for (int k : idx) in = in || k == v;
        for (int e = 0; e < 3; e++) CHECK(motvel2[(size_t)v * 3 + e] == (in ? motvel[(size_t)v * 3 + e] : -1));
        for (int e = 0; e < 51; e++) CHECK(yref2[(size_t)v * 51 + e] == (in && e < 15 ? yref[(size_t)v * 51 + e] : -1.0));
        CHECK(res2[v] == (in ? res[v] : -1.0));
    }
    for (double u : unused) CHECK(u == -1.0);

    // a contiguous shard reads and writes in place, from its first row on
    const cfn::Staged q = cfn::in_place(cfn::Layout(cols, 3, Nmax, Nmax), 4);
    CHECK(q.i(0) == motvel.data() + 12 && q.d(1) == yref.data() + 4 * 51 && q.p[2] == nullptr && q.d(3) == res.data() + 4);
    std::printf("host_rows_check ok\n");
    return 0;
}
