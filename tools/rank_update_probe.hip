// rank_update (csrc/rank_update.hip) against the K <= 32 launch of the generic GEMM it replaces, on one shape per argument
// "m,n,b": the two results are compared byte by byte, then both are timed in the same process, alternating, with a pair of
// events around each launch.  Row-major C (W with row stride n, the pitch of the reflector array of a square-ish factorisation)
// and column-major C (W with column stride m), X row-major (b x n) as in qr.hip.  Links the library's internal C++ entry points:
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/rank_update_probe.hip -Itnac4o_amd/csrc -Ltnac4o_amd -ltnpeps \
//         -Wl,-rpath,'$ORIGIN/../tnac4o_amd' -o bench_out/rank_update_probe
//   bench_out/rank_update_probe 8704,768,32 16384,992,32 [--reps 200]
// GB/s over 8 (2 m n + m b + b n) bytes; MI355X streams about 6.3 TB/s from HBM.
#include <algorithm>
#include <array>
#include <random>
#include <vector>

#include "common.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char** argv) {
    int reps = 200;
    std::vector<std::array<long, 3>> shapes;
    for (int i = 1; i < argc; ++i) {
        long m, n, b;
        if (!strcmp(argv[i], "--reps") && i + 1 < argc) reps = atoi(argv[++i]);
        else if (sscanf(argv[i], "%ld,%ld,%ld", &m, &n, &b) == 3 && m > 0 && n > 0 && b >= 1 && b <= 32) shapes.push_back({m, n, b});
        else { fprintf(stderr, "usage: %s m,n,b ... [--reps R]\n", argv[0]); return 2; }
    }
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    int bad = 0;
    for (auto& s : shapes) {
        const int64_t m = s[0], n = s[1];
        const int b = (int)s[2];
        for (int colmajor = 0; colmajor < 2; ++colmajor) {
            const int64_t wpitch = colmajor ? m : std::max<int64_t>(n, b);
            const int64_t wrs = colmajor ? 1 : wpitch, wcs = colmajor ? wpitch : 1, wlen = colmajor ? wpitch * b : m * wpitch;
            const int64_t rsc = colmajor ? 1 : n, csc = colmajor ? m : 1;
            std::vector<double> hw(wlen), hx((size_t)b * n), hc((size_t)m * n), r0(hc.size()), r1(hc.size());
            std::mt19937_64 gen(12345 + m + n + b);
            std::normal_distribution<double> nd;
            for (auto& v : hw) v = nd(gen);
            for (auto& v : hx) v = nd(gen);
            for (auto& v : hc) v = nd(gen);
            double *W, *X, *C0, *C1;
            CHECK(hipMalloc(&W, hw.size() * 8));
            CHECK(hipMalloc(&X, hx.size() * 8));
            CHECK(hipMalloc(&C0, hc.size() * 8));
            CHECK(hipMalloc(&C1, hc.size() * 8));
            CHECK(hipMemcpy(W, hw.data(), hw.size() * 8, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(X, hx.data(), hx.size() * 8, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(C0, hc.data(), hc.size() * 8, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(C1, hc.data(), hc.size() * 8, hipMemcpyHostToDevice));
            auto generic = [&]() { return tn::gemm(st, m, n, b, -1.0, W, wrs, wcs, X, n, 1, 1.0, C0, rsc, csc); };
            auto kernel = [&]() { return tn::rank_update(st, m, n, b, W, wrs, wcs, X, n, 1, C1, rsc, csc, nullptr); };
            if (generic() || kernel()) { fprintf(stderr, "launch failed: %s\n", tn::get_error()); return 2; }
            CHECK(hipStreamSynchronize(st));
            CHECK(hipMemcpy(r0.data(), C0, r0.size() * 8, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(r1.data(), C1, r1.size() * 8, hipMemcpyDeviceToHost));
            const bool same = memcmp(r0.data(), r1.data(), r0.size() * 8) == 0;
            bad += same ? 0 : 1;
            std::vector<float> tg, tk;
            for (int r = 0; r < reps + 10; ++r) {                  // (ten warm-up rounds)
                float ms;
                CHECK(hipEventRecord(e0, st));
                if (generic()) return 2;
                CHECK(hipEventRecord(e1, st));
                CHECK(hipEventSynchronize(e1));
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 10) tg.push_back(ms * 1e3f);
                CHECK(hipEventRecord(e0, st));
                if (kernel()) return 2;
                CHECK(hipEventRecord(e1, st));
                CHECK(hipEventSynchronize(e1));
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 10) tk.push_back(ms * 1e3f);
            }
            std::sort(tg.begin(), tg.end());
            std::sort(tk.begin(), tk.end());
            auto q = [&](const std::vector<float>& t, double f) { return t[(size_t)(f * (t.size() - 1))]; };
            const double bytes = 8.0 * (2.0 * m * n + (double)m * b + (double)b * n);
            printf("%6ld x %5ld x %2d %s  same bits: %s  us (min / p10 / median / p90 / max)  generic %7.1f %7.1f %7.1f %7.1f %7.1f   rank_update %7.1f %7.1f %7.1f %7.1f %7.1f"
                   "   GB/s at the median: %6.0f -> %6.0f\n",
                   (long)m, (long)n, b, colmajor ? "col-major" : "row-major", same ? "yes" : "NO", q(tg, 0), q(tg, 0.1), q(tg, 0.5), q(tg, 0.9), q(tg, 1),
                   q(tk, 0), q(tk, 0.1), q(tk, 0.5), q(tk, 0.9), q(tk, 1), bytes / q(tg, 0.5) * 1e-3, bytes / q(tk, 0.5) * 1e-3);
            fflush(stdout);
            (void)hipFree(W); (void)hipFree(X); (void)hipFree(C0); (void)hipFree(C1);
        }
    }
    return bad ? 1 : 0;
}
