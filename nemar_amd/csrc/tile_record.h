// The fixed-order record of a workgroup and its merge, for the kernels whose per-sample statistics must be the same bits on every run
// without atomics: regularity.hip (JacAcc) and similarity.hip (SimAcc).  Every lane accumulates an
// Acc; block_record folds the workgroup's into one with ONE tree — the xor tree of each wave, then the waves in ascending order — which
// the tile kernel stores as the workgroup's record in the caller's workspace; merge_records reads a sample's records in a fixed order
// and folds them with the same tree.  An Acc supplies
//   static constexpr int WORDS      the 32-bit words of a record, in LDS and in the workspace (store may leave some unused)
//   static Acc empty()              the neutral element
//   void merge(const Acc& b)        *this = *this (+) b, field by field
//   Acc shfl_xor(int o) const       the Acc of lane ^ o
//   void store(unsigned* r) const, static Acc load(const unsigned* r)
//
// Left alone on purpose: fold.hip's forward kernel spells the same tree inline for its (sum, count) pair with the wave count a
// compile-time constant — through block_record, with or without the leading barrier, nemar_fold_penalty_fwd measured 2 - 3 % slower
// (tools/profiles/eval_family_refactor.txt); fold_finish_kernel (it merges over ALL samples, with block_sum), smooth.hip, loss.hip and deform.hip's
// registration-error meter (block_sum / block_sum_u / block_max).  block_sum starts its sum over the waves from +0.f and is valid in every
// thread; block_record starts from wave 0's value and is valid in thread 0.  The two differ in the bits of a sum that is -0.f, so
// moving those files onto the record would change results.
#pragma once
#include "common.h"

namespace {

// the workgroup's total, valid in thread 0.  `red` is Acc::WORDS words of LDS per wave
template <class Acc>
__device__ __forceinline__ Acc block_record(Acc a, unsigned* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a.merge(a.shfl_xor(o));
    __syncthreads();      // protect `red` from a previous use
    if (lane == 0) a.store(red + wid * Acc::WORDS);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < nw; ++i) a.merge(Acc::load(red + i * Acc::WORDS));
    }
    return a;
}

// a sample's n_partial records merged, valid in thread 0: thread t takes records t, t + blockDim.x, ... in ascending order, then the
// workgroup's tree
template <class Acc>
__device__ __forceinline__ Acc merge_records(const unsigned* __restrict__ partial, int n_partial, unsigned* red) {
    Acc a = Acc::empty();
    for (int i = threadIdx.x; i < n_partial; i += blockDim.x) a.merge(Acc::load(partial + (size_t)i * Acc::WORDS));
    return block_record(a, red);
}

}  // namespace
