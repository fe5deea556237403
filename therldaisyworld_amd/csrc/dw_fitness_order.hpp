// dw_fitness_order.hpp — the order in which one member's rewards of one step are added: NumPy's pairwise sum, which is what
// the reference's `reward[:, :half].mean()` (daisy/evo/sges.py:170) takes over the n = worlds * half values of a member's
// block, world-major and agent-minor.  Plain C++ with no HIP header and no HIP call: fitness_means_pw (dw_fitness.hpp)
// includes it, and tests/fitness_order_driver.cpp compiles it alone and emulates the kernel's eight lanes.
//
//   n < 8          the values one by one
//   8 <= n <= 128  eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... below n - n % 8, combined as
//                  ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 leftovers one by one
//   n > 128        the sum of the first n2 = n / 2 - (n / 2) % 8 values plus the sum of the rest, each taken by this rule
//
// A range of more than 128 values is therefore a binary tree whose leaves hold 64 .. 128 values each.  The kernel has
// neither recursion nor a per-thread stack: it takes the leaves from left to right (fit_leaf_at finds each one by walking
// down from the root), keeps the sums of the finished left subtrees on a small stack, and after a leaf adds as many of
// them as subtrees end with that leaf (`closes`).  Lane j of a group of eight is accumulator r[j] (fit_lane_partial);
// three cross-lane additions at distances 1, 2, 4 are the combine tree (in every lane: floating-point addition
// commutes); the leftovers follow (fit_add_tail).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DW_FIT_HD __host__ __device__ __forceinline__
#else
#define DW_FIT_HD inline
#endif

namespace dw {

constexpr int kFitLanes = 8;          // accumulators of a leaf: lanes of a group
constexpr int kFitLeafMax = 128;      // values a leaf holds at most (NumPy's PW_BLOCKSIZE)
constexpr int kFitStackDepth = 26;    // sums that can wait at a time: n < 2^31 values are at most 25 levels above a leaf

// the split of a range of n > 128 values: the length of its left part
DW_FIT_HD int fit_split(int n) {
    const int n2 = n / 2;
    return n2 - n2 % 8;
}

struct FitLeaf {
    int lo, len;                      // the leaf's values [lo, lo + len)
    int closes;                       // subtrees that end with this leaf: sums to take from the stack behind it
};

// the leaf of a range of n values that holds value `at` (the walk asks for at = 0, then for the end of each leaf)
DW_FIT_HD FitLeaf fit_leaf_at(int n, int at) {
    int lo = 0, len = n, closes = 0;
    while (len > kFitLeafMax) {
        const int n2 = fit_split(len);
        if (at < lo + n2) {
            len = n2;
            closes = 0;
        } else {
            lo += n2;
            len -= n2;
            ++closes;
        }
    }
    return {lo, len, closes};
}

// accumulator r[j] of a leaf of len >= 8 values; load(i) is value i of the member's step
template <class Load>
DW_FIT_HD double fit_lane_partial(Load&& load, int lo, int len, int j) {
    double r = load(lo + j);
    const int body = len - len % 8;
    for (int i = 8; i < body; i += 8) r += load(lo + i + j);
    return r;
}

// the len % 8 leftovers of a leaf, added to the combined accumulators one by one
template <class Load>
DW_FIT_HD double fit_add_tail(Load&& load, int lo, int len, double res) {
    for (int i = len - len % 8; i < len; ++i) res += load(lo + i);
    return res;
}

// fewer than 8 values (and at least one): one by one
template <class Load>
DW_FIT_HD double fit_short_sum(Load&& load, int n) {
    double res = load(0);
    for (int i = 1; i < n; ++i) res += load(i);
    return res;
}

}  // namespace dw
