// dw_fitness.hpp — the fitness bookkeeping of an evolution-strategy population on the device (ref SimpleGaussianES.get_fitness,
// daisy/evo/sges.py:160-176, per member of a population evaluated as one ensemble): what harness._population_chunk does in
// NumPy on the downloaded rewards and done flags of a chunk, on the [K][B][N] arrays where the episode kernels leave them.
//
// Member block m owns worlds [m * wpm, (m + 1) * wpm); P = B / wpm.  Carried across chunks: sum_reward [P] float64,
// done_at [B][N] int32, running [P].  Three launches per chunk of K steps ("_pw": per world block):
//
//   fitness_means_pw    eight lanes per (step, member), all K * P in parallel: the mean reward of the block's agents
//                       [0, half) in NumPy's pairwise order (dw_fitness_order.hpp), divided by n = wpm * half with a correctly
//                       rounded float64 division; and whether every done flag of the block is set at that step
//   fitness_scan_pw     one thread per member, over the steps in order: whether the member runs at the start of step t
//                       (run_t), sum_reward += mean while it does, running cleared behind the step that ends it; the
//                       maximum over the members of "steps after which the member still runs" ends the chunk
//   fitness_counts_pw   one thread per (world, agent): done_at += !done over the steps at which its member runs; thread 0
//                       turns the scan's maximum into (executed, finished)
//
// No thread walks more than one member's values of one step; a member of 2000 values is 250 dependent additions per lane.
// The sums waiting for their right-hand subtrees (members of more than 128 values) live in LDS, one short stack per group
// of eight lanes: no scratch memory, no recursion.
#pragma once
#include "dw_common.hpp"
#include "dw_fitness_order.hpp"

namespace dw {

constexpr int kFitGroups = 256 / kFitLanes;                     // (step, member) pairs per workgroup of fitness_means_pw

struct FitnessArgs {
    const double* reward;             // [K][B][N]: reward * (reward > 0) of every step
    const unsigned char* done;        // [K][B][N]
    int K, B, N, wpm, half, P;
    double* means;                    // [K][P]   scratch of the chunk
    unsigned char* all_done;          // [K][P]
    unsigned char* run_t;             // [K][P]   the member runs at the start of step t
    int* out;                         // [0] steps after which some member still runs; [1] executed, [2] finished
    double* sum_reward;               // [P]      carried across chunks
    int* done_at;                     // [B][N]
    unsigned char* running;           // [P]
};

__global__ __launch_bounds__(256) void fitness_means_pw(const FitnessArgs A) {
    __shared__ double waiting[kFitGroups][kFitStackDepth];
    const int grp = threadIdx.x / kFitLanes, j = threadIdx.x % kFitLanes;
    const long long g = (long long)blockIdx.x * kFitGroups + grp;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.out[0] = 0;      // fitness_scan_pw, next on the stream, takes its maximum here
    if (g >= (long long)A.K * A.P) return;                      // (whole groups leave: the cross-lane steps stay within a group)
    const int t = (int)(g / A.P), m = (int)(g % A.P);
    const size_t bn = (size_t)A.B * A.N, first = (size_t)t * bn + (size_t)m * A.wpm * A.N;
    const double* __restrict__ rw = A.reward + first;
    const unsigned int half = (unsigned int)A.half, N = (unsigned int)A.N;
    auto load = [&](int i) { return rw[((unsigned int)i / half) * N + (unsigned int)i % half]; };   // world-major, agent-minor
    const int n = A.wpm * A.half;
    double sum;
    if (n < kFitLanes) {
        sum = fit_short_sum(load, n);
    } else {
        double* stack = waiting[grp];
        int sp = 0, at = 0;
        for (;;) {
            const FitLeaf leaf = fit_leaf_at(n, at);
            double r = fit_lane_partial(load, leaf.lo, leaf.len, j);
            r += __shfl_xor(r, 1, kFitLanes);                   // (r0 + r1), (r2 + r3), ...
            r += __shfl_xor(r, 2, kFitLanes);                   // (r0 + r1) + (r2 + r3), ...
            r += __shfl_xor(r, 4, kFitLanes);                   // every lane of the group holds the leaf's combined sum
            r = fit_add_tail(load, leaf.lo, leaf.len, r);
            for (int c = 0; c < leaf.closes; ++c) r = stack[--sp] + r;   // left subtree + right subtree
            at = leaf.lo + leaf.len;
            if (at >= n) { sum = r; break; }
            stack[sp++] = r;                                    // the eight lanes write the same value to the same place
        }
    }
    const unsigned char* __restrict__ dn = A.done + first;
    const int flags = A.wpm * A.N;
    int all = 1;
    for (int q = j; q < flags; q += kFitLanes) all &= dn[q] != 0;
    all &= __shfl_xor(all, 1, kFitLanes);
    all &= __shfl_xor(all, 2, kFitLanes);
    all &= __shfl_xor(all, 4, kFitLanes);
    if (j == 0) {
        A.means[g] = sum / (double)n;
        A.all_done[g] = (unsigned char)all;
    }
}

__global__ __launch_bounds__(256) void fitness_scan_pw(const FitnessArgs A) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= A.P) return;
    bool run = A.running[m] != 0;
    double sum = A.sum_reward[m];
    int still = 0;                                              // steps of this chunk after which the member still runs
    for (int t = 0; t < A.K; ++t) {
        const size_t i = (size_t)t * A.P + m;
        A.run_t[i] = run;
        if (run) {
            sum += A.means[i];
            if (A.all_done[i]) run = false;
            else still = t + 1;
        }
    }
    A.sum_reward[m] = sum;
    A.running[m] = run;
    atomicMax(&A.out[0], still);
}

__global__ __launch_bounds__(256) void fitness_counts_pw(const FitnessArgs A) {
    const size_t bn = (size_t)A.B * A.N, q = (size_t)blockIdx.x * 256 + threadIdx.x;
    // step `still` is the first one after which no member runs: the chunk ends with it (nothing runs at a later step)
    const int still = A.out[0], executed = still < A.K ? still + 1 : A.K;
    if (q == 0) {
        A.out[1] = executed;
        A.out[2] = still < A.K;
    }
    if (q >= bn) return;
    const int m = (int)(q / A.N) / A.wpm;
    int alive = 0;
    for (int t = 0; t < executed; ++t) alive += A.run_t[(size_t)t * A.P + m] & (A.done[(size_t)t * bn + q] == 0);
    A.done_at[q] += alive;
}

}  // namespace dw
