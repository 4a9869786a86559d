// Cross-tile mask NMS and label merge of tile-local records (util._apply_nms_tiled; reference micro_sam/util.py:1698-1747 window overlap,
// :1773-1848 merge through the global boxes): what follows batched_tiled_inference, on the bit masks of MANY tiles at once.
//
// The record table:
//   words       uint32, flat: the bit masks of all tiles one after the other, each [n, ceil(th / 32), tw] (bit b of word row yw = row
//               yw * 32 + b, tail bits zero: msam_mask_pack);
//   word_offset int64 [K]: a record's first word;
//   geom        int32 [K, 8]: wpc, tw (words per column and width of the record's tile), bx, by, bw, bh (its bbox, xywh in the tile),
//               gx, gy (where that bbox starts in the image).
// Tiles differ in shape (border tiles; heights that are no multiple of 32) and lie at arbitrary offsets from each other, so two masks
// are in general misaligned vertically by a non-multiple of 32: every address derives from the record's own wpc / tw, and 32 rows of a
// mask that start at ANY row come from the two word rows that straddle them, joined by a 64-bit shift.
//
//   overlaps : one wave per candidate pair, four pairs per workgroup; lanes over the columns of the window of the two global boxes, a
//              loop over its 32-row groups, popcount of the AND, __shfl_xor reduction.  No LDS, no barrier, no atomics.
//   paint    : label = max(label, M - r) where record order[r] is set: the FIRST record of `order` that covers a pixel wins.  A wave
//              takes (32-row group, 64-column block) items of one record: a lane aligns its column's 32 rows once, then the wave walks
//              the rows - every atomic instruction covers consecutive columns of ONE image row (256 contiguous bytes).
//
// Every word read is guarded by 0 <= wy < wpc && 0 <= x < tw, every label write by 0 <= y < H && 0 <= x < W: a malformed table reads
// zeros and writes nothing.  Integer arithmetic and integer atomicMax only: two runs give the same bits.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int TM_WGY = 4;                                              // workgroups per record of the painter (16 waves)

struct TmRec { const unsigned* w; int wpc, tw, bx, by, bw, bh, gx, gy; };

MSAM_DEVINL TmRec tm_record(const unsigned* __restrict__ words, const long long* __restrict__ word_offset, const int* __restrict__ geom, int k) {
    const int* g = geom + (size_t)k * 8;
    return TmRec{words + word_offset[k], g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7]};
}

MSAM_DEVINL unsigned tm_word(const TmRec& r, int wy, int x) {            // word row wy of column x, zero outside the tile
    return (wy >= 0 && wy < r.wpc && x >= 0 && x < r.tw) ? r.w[(size_t)wy * r.tw + x] : 0u;
}

// rows y .. y + 31 of column x (tile coordinates, any y) as one word: bit b = row y + b
MSAM_DEVINL unsigned tm_rows32(const TmRec& r, int y, int x) {
    const int wy = y >> 5, sh = y & 31;                                 // (arithmetic shift: floor for negative y)
    const unsigned lo = tm_word(r, wy, x);
    if (sh == 0) return lo;
    const unsigned long long both = ((unsigned long long)tm_word(r, wy + 1, x) << 32) | lo;
    return (unsigned)(both >> sh);
}

MSAM_DEVINL unsigned tm_first_rows(int n) { return n >= 32 ? 0xffffffffu : ((1u << n) - 1u); }    // n in [1, 32]

MSAM_DEVINL int tm_wave_add(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid ceil(Np / 4): wave w of a workgroup takes pair 4 * blockIdx.x + w
__global__ __launch_bounds__(256) void tm_overlap_kernel(const unsigned* __restrict__ words, const long long* __restrict__ word_offset,
                                                         const int* __restrict__ geom, int K, const int* __restrict__ pairs, int Np,
                                                         int* __restrict__ inter) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= Np) return;                                                // (the whole wave)
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    int count = 0;
    if (i >= 0 && i < K && j >= 0 && j < K) {
        const TmRec a = tm_record(words, word_offset, geom, i), b = tm_record(words, word_offset, geom, j);
        const int x0 = max(a.gx, b.gx), x1 = min(a.gx + a.bw, b.gx + b.bw);
        const int y0 = max(a.gy, b.gy), y1 = min(a.gy + a.bh, b.gy + b.bh);
        const int ax = a.bx - a.gx, ay = a.by - a.gy, bx = b.bx - b.gx, by = b.by - b.gy;      // image -> tile coordinates
        for (int y = y0; y < y1; y += 32) {
            const unsigned rows = tm_first_rows(y1 - y);
            for (int x = x0 + lane; x < x1; x += 64)
                count += __popc(tm_rows32(a, y + ay, x + ax) & tm_rows32(b, y + by, x + bx) & rows);
        }
    }
    count = tm_wave_add(count);
    if (lane == 0) inter[p] = count;
}

// grid (M, TM_WGY): the (32-row group, 64-column block) items of record order[blockIdx.x] strided over its 4 * TM_WGY waves
__global__ __launch_bounds__(256) void tm_paint_kernel(const unsigned* __restrict__ words, const long long* __restrict__ word_offset,
                                                       const int* __restrict__ geom, const int* __restrict__ order, int M, int H, int W,
                                                       int* __restrict__ label) {
    const int r = blockIdx.x, lane = threadIdx.x & 63;
    const int k = order[r];
    if (k < 0) return;
    const TmRec a = tm_record(words, word_offset, geom, k);
    const int value = M - r;
    const int ncb = (a.bw + 63) >> 6, items = ((a.bh + 31) >> 5) * ncb;
    for (int it = blockIdx.y * 4 + (threadIdx.x >> 6); it < items; it += 4 * TM_WGY) {
        const int dy0 = (it / ncb) * 32, dx = (it % ncb) * 64 + lane;
        const int n = min(32, a.bh - dy0), x = a.gx + dx;
        const bool col = dx < a.bw && x >= 0 && x < W;
        const unsigned bits = col ? tm_rows32(a, a.by + dy0, a.bx + dx) & tm_first_rows(n) : 0u;
        for (int q = 0; q < n; ++q) {                                   // one image row per step, consecutive columns across the wave
            const int y = a.gy + dy0 + q;
            if (((bits >> q) & 1u) && y >= 0 && y < H) atomicMax(label + (size_t)y * W + x, value);
        }
    }
}

bool tm_table_ok(const void* words, const void* word_offset, const void* geom) { return words && word_offset && geom; }

}  // namespace

extern "C" int msam_tiled_mask_overlaps(const uint32_t* words, const int64_t* word_offset, const int32_t* geom, int32_t K,
                                        const int32_t* pairs, int32_t Np, int32_t* inter, void* stream) {
    if (K < 0 || Np < 0 || (Np > 0 && (!tm_table_ok(words, word_offset, geom) || !pairs || !inter || K == 0))) {
        msam_set_error("msam_tiled_mask_overlaps: bad arguments");
        return 1;
    }
    if (Np == 0) return 0;
    hipLaunchKernelGGL(tm_overlap_kernel, dim3((Np + 3) / 4), dim3(256), 0, (hipStream_t)stream, words, (const long long*)word_offset,
                       geom, K, pairs, Np, inter);
    return msam_check_launch("msam_tiled_mask_overlaps");
}

extern "C" int msam_paint_tiled(const uint32_t* words, const int64_t* word_offset, const int32_t* geom, const int32_t* order, int32_t M,
                                int32_t H, int32_t W, int32_t* label, void* stream) {
    if (!label || H <= 0 || W <= 0 || M < 0 || (M > 0 && (!tm_table_ok(words, word_offset, geom) || !order))) {
        msam_set_error("msam_paint_tiled: bad arguments");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(label, 0, (size_t)H * W * sizeof(int), s) != hipSuccess) { msam_set_error("msam_paint_tiled: memset failed"); return 2; }
    if (M == 0) return 0;
    hipLaunchKernelGGL(tm_paint_kernel, dim3(M, TM_WGY), dim3(256), 0, s, words, (const long long*)word_offset, geom, order, M, H, W, label);
    return msam_check_launch("msam_paint_tiled");
}
