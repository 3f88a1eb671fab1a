// Counting into a workgroup's LDS table from whole waves: score.hip (nemar_label_overlap: per-class counters) and similarity.hip
// (nemar_joint_histogram: the bins x bins table) share one statement of it.
#pragma once
#include "common.h"

namespace {

// hist[key] += 1 from every lane with key >= 0 (the whole wave calls this together): the lanes that hold the first counting lane's key
// are added by that lane alone.  per_lane (a launch argument: the same kernel in both builds of the library): every
// lane adds for itself
__device__ __forceinline__ void wave_count(unsigned* hist, int key, int per_lane) {
    const bool counts = key >= 0;
    if (per_lane) {                                               // (wave-uniform)
        if (counts) atomicAdd(&hist[key], 1u);
        return;
    }
    const unsigned long long active = __ballot(counts);
    if (active == 0ull) return;                                   // (wave-uniform)
    const int leader = __builtin_ctzll(active);
    const int lead_key = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(counts && key == lead_key);
    const int lane = threadIdx.x & 63;
    if (lane == leader) atomicAdd(&hist[lead_key], (unsigned)__builtin_popcountll(same));
    else if (counts && key != lead_key) atomicAdd(&hist[key], 1u);
}

}  // namespace
