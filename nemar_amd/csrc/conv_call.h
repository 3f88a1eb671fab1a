// The side inputs and outcomes of ONE convolution call (conv.hip's operators and the wide-layer route behind them).  A ConvCall lives on
// the stack of the C-ABI entry point for the duration of the call and is passed down by reference: the plain entry points start from an
// empty one, the _ex entry points copy the members of nemar_conv_extras (include/nemar_hip.h) their operator documents.
#pragma once
#include <stddef.h>

// max |t| words the caller computed for a source tensor: one per sample (count == N) or one for the whole tensor (count == 1)
struct MaxWords {
    const unsigned* words = nullptr;
    int count = 0;
};

struct ConvCall {
    // ---- inputs (all optional) ----
    void* scratch = nullptr;              // transient arena of the wide-layer route
    size_t scratch_bytes = 0;
    MaxWords src_max;                     // source = x0 (fwd, bwd_weight) / gy (bwd_data)
    MaxWords src2_max;                    // bwd_weight: gy
    const void* src_planes = nullptr;     // fwd / bwd_data: the source's channel-blocked planes, holding ...
    int src_planes_kind = -1;             // ... this SPLIT16_* content (conv_split16.h)
    const void* x_planes = nullptr;       // bwd_weight: the pixel-major X planes of x0 a forward producer wrote
    void* gy_planes_out = nullptr;        // bwd_data: where the pass that splits gy also leaves the weight gradient's planes
    size_t gy_planes_bytes = 0;
    const void* src2_planes = nullptr;    // bwd_weight: those planes
    const float* addend = nullptr;        // bwd_data: tensor added to gx0 in the epilogue
    void* out_max = nullptr;              // bwd_data: per-sample max |gx0| words
    const float* bias_partials = nullptr; // bwd_weight: per-plane sums of gy [N, K]
    // ---- outcomes (set by the route that ran) ----
    bool gy_planes_written = false;       // gy_planes_out was filled
    bool epilogue_fused = false;          // addend and out_max were both honoured (the wide route's epilogue)
    bool addend_done = false;             // the addend alone was (a fold pass)
    bool bias_rode = false;               // bias_partials were reduced inside the slab-sum launch
};
