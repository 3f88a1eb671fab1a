// Scoring a registration's boundaries (DESIGN.md "Surface distances"): the distances between the class boundaries of the warped moving
// label map m and of the fixed label map f, from which the Hausdorff distance, HD95 and the average symmetric surface distance follow.
// Not a call site of the reference, which has no evaluation code.  m(x) is the class of the value nemar_warp_resampled_fwd(NEAREST)
// would write — pred_view / taps_at<SAMPLE_NEAREST> of resampled_grid.h, as score.hip's label_overlap_kernel reads it.
//
//   nemar_surface_distance   per sample, class and direction: the number of boundary pixels, the histogram of their squared distances
//                            to the other map's boundary of the same class (bins d2 < max_dist^2), the number beyond it (`far`) and the
//                            largest d2; optionally the d2 of every boundary pixel as a map.
//
// Squared pixel distances are integers: every result is exact, added with integer atomics (order-free, bitwise repeatable), and there
// is no float arithmetic after the warp's own coordinate.  The passes (workspace planes are 16 bits per pixel):
//   0a  class_kernel     tiles of pred_view: raw[0] = class of m, raw[1] = class of f (NONE where the value is of no class)
//   0b  boundary_kernel  code = class | BOUNDARY where a 4-neighbour (or the plane's edge) is not of the pixel's class; boundary pixels
//                        per class counted with wave_count into LDS, flushed to counts[n,k,dir,0]; dist2 = -1 off the boundaries
//   1   column_kernel    per class of the chunk (a grid dimension), map and 64-column strip: g(y,x) = the vertical distance from (y,x)
//                        to the nearest boundary pixel of class k in column x (COL_INF: none), a sweep down and a sweep up per quarter
//                        of the rows; lanes on consecutive x.  A class without boundary pixels in either map returns at once (counts
//                        read on the device)
//   2   row_kernel       one sweep of the codes per chunk: at a boundary pixel (y,x) of class k of the chunk, in the OTHER map's g,
//                        d2 = min over x' of (x - x')^2 + g(y,x')^2, searched outwards from x; into hist / far / max d2 / dist2,
//                        added up per tile and per workgroup in LDS first
// The g planes of a chunk take at most G_BYTES (or one class, if one class alone is larger): nemar_surface_distance_workspace says so.
#include "common.h"
#include "pred_launch.h"
#include "wave_count.h"

namespace {

constexpr int MAX_CLASSES = 1024;          // score.hip's: a class fits the low 15 bits of a code
constexpr int MAX_DIST = 128;              // bins = max_dist^2 <= 16384 per (sample, class, direction)
constexpr int MAX_SIDE = 32768;            // d2 <= 2 * 32767^2 < 2^31: an int, and an unsigned that is never NO_DIST
constexpr unsigned short NONE = 0x7fff, BOUNDARY = 0x8000, COL_INF = 0xffff;
constexpr unsigned NO_DIST = 0xffffffffu;
constexpr size_t G_BYTES = (size_t)128 << 20;      // the bound on a chunk's g planes
constexpr int COLS = 64;                   // columns of a column_kernel workgroup: a wave's lanes
constexpr int COL_WAVES = 4, COL_BATCH = 8;
constexpr int ROW_BATCH = 8;               // horizontal distances per round of row_search's loads
constexpr int ROW_SLOTS = 512;             // a row_kernel workgroup's table of (class, direction, d2) keys: a power of two
constexpr int NO_ROW = 1 << 20;            // no boundary row: farther than any row of a plane from any other (a side is at most 32768)

__device__ __forceinline__ int nemar_cdiv_dev(int a, int b) { return (a + b - 1) / b; }

// class of a label value (score.hip's class_of rule): k iff v == (float)k for an integer 0 <= k < K; anything else is -1
__device__ __forceinline__ int class_of(float v, int K) {
    if (!(v >= 0.f && v < (float)K)) return -1;
    const int k = (int)v;
    return (float)k == v ? k : -1;
}

// counts [N,K,2,3]: (boundary pixels, far, max d2) of direction 0 (m -> f: the pixels are m's) and 1 (f -> m)
__device__ __forceinline__ size_t count_at(int n, int K, int k, int dir) { return (((size_t)n * K + k) * 2 + dir) * 3; }

// ---- pass 0a: both class maps ----
template <int MODE, bool RESAMPLE>
__global__ __launch_bounds__(RT_THREADS) void class_kernel(const float* __restrict__ lm, const float* __restrict__ lf,
                                                           const float* __restrict__ pred, unsigned short* __restrict__ raw, int N, int K,
                                                           int Hs, int Ws, int hf, int wf, int Ho, int Wo, float sh, float sw, int tiles_x,
                                                           int tiles) {
    __shared__ float patch[RESAMPLE ? 2 * RT_PH * RT_PW : 1];
    const int n = blockIdx.y, tid = threadIdx.x;
    const auto pv = pred_view<MODE, RESAMPLE>(pred, n, hf, wf, Ho, Wo, sh, sw);
    const float* lmN = lm + (size_t)n * Hs * Ws;
    const float* lfN = lf + (size_t)n * pv.oplane;
    unsigned short* rm = raw + (size_t)n * pv.oplane;
    unsigned short* rf = raw + ((size_t)N + n) * pv.oplane;
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tyi = t / tiles_x;
        const int x0 = (t - tyi * tiles_x) * RT_W, y0 = tyi * RT_H;
        if (RESAMPLE) __syncthreads();                            // the previous tile's readers are done with the patch
        const FieldPatch fp = pv.stage(patch, x0, y0, tid);
        if (RESAMPLE) __syncthreads();
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
            if (h < Ho && w < Wo) {
                float gx, gy;
                pv.coord(patch, fp, h, w, gx, gy);
                const Taps tp = taps_at<SAMPLE_NEAREST>(gx, gy, Ws, Hs);
                const int km = class_of(sample_at<SAMPLE_NEAREST>(lmN, tp), K);
                const size_t o = (size_t)h * Wo + w;
                const int kf = class_of(lfN[o], K);
                rm[o] = km < 0 ? NONE : (unsigned short)km;
                rf[o] = kf < 0 ? NONE : (unsigned short)kf;
            }
        }
    }
}

// ---- pass 0b: boundary flags and boundary pixels per class ----
__global__ __launch_bounds__(RT_THREADS) void boundary_kernel(const unsigned short* __restrict__ raw, unsigned short* __restrict__ code,
                                                              unsigned* __restrict__ counts, int* __restrict__ dist2, int N, int K, int Ho,
                                                              int Wo, int tiles_x, int tiles) {
    __shared__ unsigned hist[2 * MAX_CLASSES];                    // [0,K) m, [K,2K) f
    const int n = blockIdx.y, tid = threadIdx.x;
    const size_t plane = (size_t)Ho * Wo;
    for (int e = tid; e < 2 * K; e += RT_THREADS) hist[e] = 0u;
    __syncthreads();
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {         // (the same trip count in every lane of the workgroup)
        const int tyi = t / tiles_x;
        const int x0 = (t - tyi * tiles_x) * RT_W, y0 = tyi * RT_H;
#pragma unroll
        for (int i = 0; i < RUNS; ++i) {
            const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
            const bool inside = h < Ho && w < Wo;                 // (no early exit: the whole wave reaches the ballots)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                int key = -1;
                if (inside) {
                    const size_t pl = ((size_t)s * N + n) * plane, o = (size_t)h * Wo + w;
                    const unsigned short* r = raw + pl;
                    const unsigned short c = r[o];
                    // a neighbour outside the plane is not of the class
                    const bool edge = c != NONE && (w == 0 || r[o - 1] != c || w == Wo - 1 || r[o + 1] != c || h == 0 || r[o - Wo] != c ||
                                                    h == Ho - 1 || r[o + Wo] != c);
                    code[pl + o] = edge ? (unsigned short)(c | BOUNDARY) : c;
                    if (edge) key = c;
                    else if (dist2) dist2[((size_t)n * 2 + s) * plane + o] = -1;
                }
                wave_count(hist + s * K, key, 0);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < 2 * K; e += RT_THREADS) {
        const unsigned v = hist[e];
        const int s = e / K, k = e - s * K;
        if (v) atomicAdd(&counts[count_at(n, K, k, s)], v);
    }
}

// ---- pass 1: vertical distances to the boundary of class k0 + blockIdx.y / 2 in map blockIdx.y % 2 ----
// A workgroup owns 64 columns, lane = column, and its COL_WAVES waves a quarter of the rows each.  First every wave finds the first and the
// last boundary row of its quarter (loads only, nothing depends on them: they overlap); the waves exchange these through LDS, so that each
// knows the nearest boundary row above and below its quarter; then a sweep down writes the distance to the nearest boundary row at or
// above, and a sweep up lowers it to the distance to the nearest at or below where that is smaller.  The sweeps load COL_BATCH rows ahead
// of the arithmetic that chains them.
__global__ __launch_bounds__(COLS * COL_WAVES) void column_kernel(const unsigned short* __restrict__ code, const unsigned* __restrict__ counts,
                                                                  unsigned short* __restrict__ g, int N, int K, int k0, int Ho, int Wo) {
    __shared__ int firsts[COL_WAVES][COLS], lasts[COL_WAVES][COLS];
    const int n = blockIdx.z, kc = blockIdx.y >> 1, s = blockIdx.y & 1, k = k0 + kc;
    // the pair is not defined: nobody reads this plane (workgroup-uniform, from device memory)
    if (counts[count_at(n, K, k, 0)] == 0u || counts[count_at(n, K, k, 1)] == 0u) return;
    const int lane = threadIdx.x % COLS, wv = threadIdx.x / COLS;
    const int x = blockIdx.x * COLS + lane;
    const bool live = x < Wo;                                     // (no early exit: the barrier below)
    const size_t plane = (size_t)Ho * Wo;
    const unsigned short* c = code + ((size_t)s * N + n) * plane + (live ? x : 0);
    unsigned short* gp = g + (((size_t)kc * 2 + s) * N + n) * plane + (live ? x : 0);
    const unsigned short want = (unsigned short)(k | BOUNDARY);
    const int rows = nemar_cdiv_dev(Ho, COL_WAVES), ya = min(wv * rows, Ho), yb = min(ya + rows, Ho);
    int first = NO_ROW, last = -NO_ROW;
#pragma unroll 8
    for (int y = ya; y < yb; ++y) {
        if (c[(size_t)y * Wo] == want) {
            first = min(first, y);
            last = y;
        }
    }
    firsts[wv][lane] = first;
    lasts[wv][lane] = last;
    __syncthreads();
    int prev = -NO_ROW, next = NO_ROW;                            // the nearest boundary row above / below this wave's rows
    for (int w = 0; w < COL_WAVES; ++w) {
        if (w < wv) prev = max(prev, lasts[w][lane]);
        if (w > wv) next = min(next, firsts[w][lane]);
    }
    if (!live) return;
    for (int y0 = ya; y0 < yb; y0 += COL_BATCH) {
        unsigned short v[COL_BATCH];
#pragma unroll
        for (int j = 0; j < COL_BATCH; ++j) v[j] = y0 + j < yb ? c[(size_t)(y0 + j) * Wo] : (unsigned short)0;
#pragma unroll
        for (int j = 0; j < COL_BATCH; ++j) {
            const int y = y0 + j;
            if (v[j] == want) prev = y;                           // (a row past yb holds 0, which is no boundary code)
            if (y < yb) gp[(size_t)y * Wo] = (unsigned short)min(y - prev, (int)COL_INF);
        }
    }
    for (int y0 = yb - 1; y0 >= ya; y0 -= COL_BATCH) {
        unsigned short v[COL_BATCH];
#pragma unroll
        for (int j = 0; j < COL_BATCH; ++j) v[j] = y0 - j >= ya ? gp[(size_t)(y0 - j) * Wo] : (unsigned short)1;
#pragma unroll
        for (int j = 0; j < COL_BATCH; ++j) {
            const int y = y0 - j;
            if (v[j] == 0) next = y;                              // (a row before ya reads as 1: not a boundary row)
            const int up = min(next - y, (int)COL_INF);
            if (y >= ya && up < (int)v[j]) gp[(size_t)y * Wo] = (unsigned short)up;
        }
    }
}

// ---- pass 2: the squared distance of every boundary pixel whose class is in [k0, k0 + kn) ----
// d2 of the boundary pixel (h, w) from `row`, row h of the other map's g plane of its class: min over x' of (w - x')^2 + g(h, x')^2
__device__ __forceinline__ unsigned row_search(const unsigned short* __restrict__ row, int w, int Wo) {
    const unsigned v0 = row[w];
    unsigned best = v0 == COL_INF ? NO_DIST : v0 * v0;
    // Outwards from x.  A column at horizontal distance >= r costs at least r * r, whatever its g; so once r * r >= best no column not
    // yet visited can be nearer than best: the stop is exact.  The columns are taken ROW_BATCH distances at a time, so that their loads
    // overlap; those of a batch beyond the stop cost at least best and change nothing.  (The pair is defined, so some column of the
    // row is finite — g of a column that holds a boundary pixel is finite in every row — and best ends finite.)
    for (int r0 = 1; r0 < Wo && (unsigned)r0 * (unsigned)r0 < best; r0 += ROW_BATCH) {
        unsigned vl[ROW_BATCH], vr[ROW_BATCH];
#pragma unroll
        for (int j = 0; j < ROW_BATCH; ++j) {
            const int r = r0 + j;
            vl[j] = w - r >= 0 ? row[w - r] : COL_INF;
            vr[j] = w + r < Wo ? row[w + r] : COL_INF;
        }
#pragma unroll
        for (int j = 0; j < ROW_BATCH; ++j) {
            const unsigned rr = (unsigned)(r0 + j) * (unsigned)(r0 + j);
            if (vl[j] != COL_INF) best = min(best, rr + vl[j] * vl[j]);
            if (vr[j] != COL_INF) best = min(best, rr + vr[j] * vr[j]);
        }
    }
    return best;
}

// Neighbouring boundary pixels have the same few distances, and global atomics on one address take turns: a workgroup adds up what a
// tile holds before it goes to `hist`.  A key is (class of the chunk, direction, d2); per tile every key bids for the slot of its low bits
// with an LDS atomicMax, the keys that hold their slot after the barrier count into it, the others add to `hist` themselves, and the
// slots are flushed with one global add each.  `far` and the largest d2 are kept per class and direction for the whole workgroup.
__global__ __launch_bounds__(RT_THREADS) void row_kernel(const unsigned short* __restrict__ code, const unsigned short* __restrict__ g,
                                                         unsigned* __restrict__ counts, unsigned* __restrict__ hist, int* __restrict__ dist2,
                                                         int N, int K, int k0, int kn, int B, int Ho, int Wo, int tiles_x, int tiles) {
    __shared__ unsigned any_boundary;
    __shared__ unsigned slot_key[ROW_SLOTS], slot_count[ROW_SLOTS];          // key + 1 (0: free), pixels
    __shared__ unsigned far_l[2 * MAX_CLASSES], max_l[2 * MAX_CLASSES];       // [class of the chunk][direction]
    const int n = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) any_boundary = 0u;
    for (int e = tid; e < 2 * kn; e += RT_THREADS) far_l[e] = max_l[e] = 0u;
    __syncthreads();
    for (int e = tid; e < kn; e += RT_THREADS) {
        const unsigned in_m = counts[count_at(n, K, k0 + e, 0)], in_f = counts[count_at(n, K, k0 + e, 1)];
        if ((in_m != 0u && in_f != 0u) || (dist2 && (in_m | in_f) != 0u)) atomicOr(&any_boundary, 1u);
    }
    __syncthreads();
    // no class of the chunk is defined in this sample, and none owes a -2 to the map: the plane is not swept
    if (!any_boundary) return;
    const size_t plane = (size_t)Ho * Wo;
    unsigned* histN = hist + ((size_t)n * K + k0) * 2 * B;                    // + key: [class of the chunk][direction][d2]
    constexpr int ROWS = RT_THREADS / RT_W, RUNS = RT_H / ROWS;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                     // (the same trip count in every lane of the workgroup)
        const int tyi = t / tiles_x;
        const int x0 = (t - tyi * tiles_x) * RT_W, y0 = tyi * RT_H;
        for (int e = tid; e < ROW_SLOTS; e += RT_THREADS) slot_key[e] = slot_count[e] = 0u;      // (flushed by this same lane)
        __syncthreads();
        int key[2 * RUNS];
#pragma unroll
        for (int j = 0; j < 2 * RUNS; ++j) {
            const int i = j >> 1, s = j & 1;
            const int h = y0 + tid / RT_W + ROWS * i, w = x0 + tid % RT_W;
            key[j] = -1;
            if (h < Ho && w < Wo) {
                const size_t o = (size_t)h * Wo + w;
                const unsigned short c = code[((size_t)s * N + n) * plane + o];
                const int kc = (c & NONE) - k0;
                if ((c & BOUNDARY) && kc >= 0 && kc < kn) {
                    if (counts[count_at(n, K, k0 + kc, 1 - s)] == 0u) {       // the other map has no boundary of this class
                        if (dist2) dist2[((size_t)n * 2 + s) * plane + o] = -2;
                    } else {
                        const unsigned best = row_search(g + (((size_t)kc * 2 + (1 - s)) * N + n) * plane + (size_t)h * Wo, w, Wo);
                        if (best < (unsigned)B) {
                            key[j] = (kc * 2 + s) * B + (int)best;
                            atomicMax(&slot_key[key[j] & (ROW_SLOTS - 1)], (unsigned)key[j] + 1u);
                        } else {
                            atomicAdd(&far_l[kc * 2 + s], 1u);
                        }
                        atomicMax(&max_l[kc * 2 + s], best);
                        if (dist2) dist2[((size_t)n * 2 + s) * plane + o] = (int)best;
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2 * RUNS; ++j) {
            if (key[j] >= 0) {
                const int slot = key[j] & (ROW_SLOTS - 1);
                if (slot_key[slot] == (unsigned)key[j] + 1u) atomicAdd(&slot_count[slot], 1u);
                else atomicAdd(&histN[key[j]], 1u);
            }
        }
        __syncthreads();
        for (int e = tid; e < ROW_SLOTS; e += RT_THREADS)
            if (slot_count[e]) atomicAdd(&histN[slot_key[e] - 1u], slot_count[e]);
    }
    __syncthreads();
    for (int e = tid; e < 2 * kn; e += RT_THREADS) {
        unsigned* cnt = counts + count_at(n, K, k0 + (e >> 1), e & 1);
        if (far_l[e]) atomicAdd(&cnt[1], far_l[e]);
        if (max_l[e]) atomicMax(&cnt[2], max_l[e]);
    }
}

// classes per chunk: as many as G_BYTES of g planes hold (two 16-bit planes per class and sample), at least one
size_t chunk_classes(int N, int K, int Ho, int Wo) {
    const size_t per_class = (size_t)4 * N * Ho * Wo;
    const size_t fit = G_BYTES / per_class;
    return fit < 1 ? 1 : (fit > (size_t)K ? (size_t)K : fit);
}
size_t map_bytes(int N, int Ho, int Wo) { return (size_t)4 * N * Ho * Wo; }     // two 16-bit planes per sample

bool shape_ok(int N, int K, int Ho, int Wo) { return N > 0 && K >= 1 && K <= MAX_CLASSES && Ho > 0 && Wo > 0 && Ho <= MAX_SIDE && Wo <= MAX_SIDE; }

}  // namespace

// raw class maps + coded class maps + the g planes of one chunk
NEMAR_API size_t nemar_surface_distance_workspace(int N, int K, int Ho, int Wo) {
    if (!shape_ok(N, K, Ho, Wo)) return 0;
    return 2 * map_bytes(N, Ho, Wo) + chunk_classes(N, K, Ho, Wo) * map_bytes(N, Ho, Wo);
}

NEMAR_API int nemar_surface_distance(const float* labels_moving, const float* labels_fixed, const float* pred, int grid_mode, unsigned* counts,
                                     unsigned* hist, int* dist2, void* workspace, size_t workspace_bytes, int N, int K, int max_dist, int Hs,
                                     int Ws, int hf, int wf, int Ho, int Wo, void* stream) {
    NEMAR_CLEAR_HIP_ERROR();
    NEMAR_REQUIRE(labels_moving && labels_fixed && pred && counts && hist && workspace, "surface_distance: null pointer");
    NEMAR_REQUIRE(((((uintptr_t)labels_moving) | ((uintptr_t)labels_fixed) | ((uintptr_t)pred) | ((uintptr_t)counts) | ((uintptr_t)hist) |
                    ((uintptr_t)dist2) | ((uintptr_t)workspace)) & 3) == 0,
                  "surface_distance: labels_moving, labels_fixed, pred, counts, hist, dist2 and workspace must be 4-byte aligned");
    NEMAR_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "surface_distance: bad shape N=%d source %dx%d output %dx%d", N, Hs, Ws, Ho, Wo);
    NEMAR_REQUIRE(K >= 1 && K <= MAX_CLASSES, "surface_distance: %d classes (1 .. %d)", K, MAX_CLASSES);
    NEMAR_REQUIRE(max_dist >= 1 && max_dist <= MAX_DIST, "surface_distance: max_dist %d (1 .. %d)", max_dist, MAX_DIST);
    NEMAR_REQUIRE(Ho <= MAX_SIDE && Wo <= MAX_SIDE, "surface_distance: output %dx%d (a side of at most %d: squared distances fit 31 bits)", Ho, Wo,
                  MAX_SIDE);
    NEMAR_REQUIRE((long long)Hs * Ws < (1ll << 31), "surface_distance: source plane too large");
    NEMAR_REQUIRE_OK(pred_ok("surface_distance", "", grid_mode, hf, wf) && tile_grid_ok("surface_distance", N, Ho, Wo));
    const size_t need = nemar_surface_distance_workspace(N, K, Ho, Wo);
    NEMAR_REQUIRE(workspace_bytes >= need, "surface_distance: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int B = max_dist * max_dist;
    NEMAR_HIP_CALL(hipMemsetAsync(counts, 0, (size_t)N * K * 6 * sizeof(unsigned), st));
    NEMAR_HIP_CALL(hipMemsetAsync(hist, 0, (size_t)N * K * 2 * B * sizeof(unsigned), st));
    unsigned short* raw = (unsigned short*)workspace;
    unsigned short* code = raw + (size_t)2 * N * Ho * Wo;
    unsigned short* g = code + (size_t)2 * N * Ho * Wo;
    const int tiles_x = nemar_cdiv(Wo, RT_W), tiles = tiles_x * nemar_cdiv(Ho, RT_H);
    const dim3 walk(resident_groups(N, 8, tiles), N), block(RT_THREADS);
    dispatch_pred(grid_mode, hf, wf, Ho, Wo, [&](auto mode, auto resample, int hf, int wf, float sh, float sw) {
        hipLaunchKernelGGL((class_kernel<decltype(mode)::value, decltype(resample)::value>), walk, block, 0, st, labels_moving, labels_fixed, pred, raw,
                           N, K, Hs, Ws, hf, wf, Ho, Wo, sh, sw, tiles_x, tiles);
    });
    hipLaunchKernelGGL(boundary_kernel, walk, block, 0, st, (const unsigned short*)raw, code, counts, dist2, N, K, Ho, Wo, tiles_x, tiles);
    const int chunk = (int)chunk_classes(N, K, Ho, Wo);
    for (int k0 = 0; k0 < K; k0 += chunk) {
        const int kn = K - k0 < chunk ? K - k0 : chunk;
        hipLaunchKernelGGL(column_kernel, dim3(nemar_cdiv(Wo, COLS), 2 * kn, N), dim3(COLS * COL_WAVES), 0, st, (const unsigned short*)code,
                           (const unsigned*)counts, g, N, K, k0, Ho, Wo);
        hipLaunchKernelGGL(row_kernel, walk, block, 0, st, (const unsigned short*)code, (const unsigned short*)g, counts, hist, dist2, N, K, k0, kn,
                           B, Ho, Wo, tiles_x, tiles);
    }
    NEMAR_CHECK_LAUNCH("surface_distance");
    return NEMAR_OK;
}
