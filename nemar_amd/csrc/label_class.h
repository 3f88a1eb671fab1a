// What a class is in a label map: one statement for the score (score.hip: nemar_label_overlap counts it) and for the loss that trains
// against it (dice.hip), so that the number that is reported and the number that is trained against cannot drift apart.
#pragma once
#include "common.h"

namespace {

constexpr int MAX_CLASSES = 1024;          // the per-workgroup class tables of score.hip and dice.hip are sized for it

// class of a label value: k iff v == (float)k for an integer 0 <= k < K; anything else (negative, >= K, fractional, NaN, Inf) is -1
__device__ __forceinline__ int class_of(float v, int K) {
    if (!(v >= 0.f && v < (float)K)) return -1;
    const int k = (int)v;
    return (float)k == v ? k : -1;
}

}  // namespace
