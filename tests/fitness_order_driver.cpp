// fitness_order_driver.cpp — the order of fitness_means_pw's sums without a GPU (tests/test_fitness_device_cpu.py).
// Includes only csrc/dw_fitness_order.hpp and does what a group of eight lanes of the kernel does, the lanes one after the
// other: lane j is accumulator r[j] of a leaf, three rounds of additions at lane distances 1, 2, 4 are the combine tree, the
// leftovers follow, and the sums of finished left subtrees wait on a small stack.
//
//   fitness_order_driver VALUES.f64 n [n ...]
//
// VALUES.f64 holds float64 values in the machine's byte order.  For every n (at most the number of values): one line
// "n <bits of the sum of the first n values> <bits of that sum / n>", the bits as 16 hexadecimal digits.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dw_fitness_order.hpp"

static double lanes_sum(const std::vector<double>& a, int n) {
    auto load = [&](int i) { return a[(size_t)i]; };
    if (n < dw::kFitLanes) return dw::fit_short_sum(load, n);
    double stack[dw::kFitStackDepth];
    int sp = 0, at = 0;
    for (;;) {
        const dw::FitLeaf leaf = dw::fit_leaf_at(n, at);
        if (leaf.lo != at || leaf.len < dw::kFitLanes || leaf.len > dw::kFitLeafMax) {
            std::fprintf(stderr, "leaf [%d, +%d) asked for at %d of %d\n", leaf.lo, leaf.len, at, n);
            std::exit(3);
        }
        double r[dw::kFitLanes], x[dw::kFitLanes];
        for (int j = 0; j < dw::kFitLanes; ++j) r[j] = dw::fit_lane_partial(load, leaf.lo, leaf.len, j);
        for (int d = 1; d < dw::kFitLanes; d *= 2) {              // every lane adds the value of lane j ^ d to its own
            for (int j = 0; j < dw::kFitLanes; ++j) x[j] = r[j ^ d];
            for (int j = 0; j < dw::kFitLanes; ++j) r[j] += x[j];
        }
        for (int j = 1; j < dw::kFitLanes; ++j)
            if (std::memcmp(&r[j], &r[0], sizeof(double)) != 0) {
                std::fprintf(stderr, "lane %d disagrees with lane 0 behind the combine\n", j);
                std::exit(3);
            }
        double res = dw::fit_add_tail(load, leaf.lo, leaf.len, r[0]);
        for (int c = 0; c < leaf.closes; ++c) {
            if (sp == 0) { std::fprintf(stderr, "empty stack\n"); std::exit(3); }
            res = stack[--sp] + res;
        }
        at = leaf.lo + leaf.len;
        if (at >= n) {
            if (sp != 0) { std::fprintf(stderr, "%d sums left on the stack\n", sp); std::exit(3); }
            return res;
        }
        if (sp == dw::kFitStackDepth) { std::fprintf(stderr, "stack overflow\n"); std::exit(3); }
        stack[sp++] = res;
    }
}

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s VALUES.f64 n [n ...]\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<double> a;
    double buf[512];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 512, f)) > 0) a.insert(a.end(), buf, buf + got);
    std::fclose(f);
    for (int i = 2; i < argc; ++i) {
        const long n = std::strtol(argv[i], nullptr, 10);
        if (n < 1 || (size_t)n > a.size()) {
            std::fprintf(stderr, "n = %ld outside 1..%zu\n", n, a.size());
            return 2;
        }
        const double s = lanes_sum(a, (int)n);
        std::printf("%ld %016" PRIx64 " %016" PRIx64 "\n", n, bits(s), bits(s / (double)n));
    }
    return 0;
}
