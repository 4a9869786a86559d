// Device side of the slice-to-slice propagation of many objects (multi_dimensional_segmentation.segment_objects_in_volume; reference
// micro_sam/multi_dimensional_segmentation.py:105-233 + prompt_based_segmentation.py:30-35, :84-115, :123-145): what happens between two
// batched decodes of consecutive slices, on the bit masks msam_postprocess_masks leaves in HBM.
//
// Layout of every mask stack here: uint32 [P, ceil(H / 32), W], bit b of word [p][yw][x] = pixel (yw * 32 + b, x): consecutive x are
// consecutive words, so one lane per column reads coalesced.  Bits of rows >= H in the last word row are IGNORED by every entry point
// (masked with tail_mask) and may hold anything.
//
//   pack    : uint8 [P, H, W] (== 1) -> bit masks; one lane per (word row, column), 32 coalesced row reads.
//   iou     : popcount of AND / OR per word, wave reduction, LDS across the four waves, one integer atomic pair per workgroup into
//             counts [P, 2]; a second launch turns them into the keep flags with the fp64 expression of util.compute_iou.
//   box     : per column the first / last set row, wave min / max, four integer atomics per wave that holds a set pixel - accumulated IN
//             the float32 [P, 4] output viewed as int32 -, then one thread per object finishes the box in fp64 (extension, clip, round half
//             to even, scale to the model's input frame, round to fp32).
//   logits  : antialiased bilinear resize of the binary mask to get_preprocess_shape(H, W, 256), zero padding, threshold at 0.5.  One
//             lane per (output column, band of 8 output rows): per source word row the horizontal taps accumulate 32 rows at once from the
//             32 bits of every tap's word, the vertical taps of the band's rows are applied to those 32 sums in registers.  No LDS.
//   paint   : label = max(label, id[p]) where bit p is set and keep[p] != 0; one lane per (word row, column), 32 running maxima.
//
// Integer sums and integer atomics only (the float work of the resize is private to a lane): two runs give the same bits.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int PR_INF = 0x7fffffff;
constexpr int PR_BAND = 8;                                             // output rows of the resize per lane
constexpr int PR_SIDE = 256;                                           // side of the mask prompt

MSAM_DEVINL unsigned tail_mask(int H, int yw) {                        // the bits of word row yw that are rows of the image
    const int left = H - yw * 32;
    return left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
}

MSAM_DEVINL int wave_add(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

MSAM_DEVINL int wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}

MSAM_DEVINL int wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// grid (ceil(W / 256) * WPC, P)
__global__ __launch_bounds__(256) void pr_pack_kernel(const unsigned char* __restrict__ masks, int H, int W, int WPC, int XB,
                                                      unsigned* __restrict__ bits) {
    const int p = blockIdx.y, yw = blockIdx.x / XB, x = (blockIdx.x - yw * XB) * 256 + threadIdx.x;
    if (x >= W) return;
    const unsigned char* __restrict__ src = masks + ((size_t)p * H + (size_t)yw * 32) * W + x;
    const int rows = H - yw * 32 < 32 ? H - yw * 32 : 32;
    unsigned word = 0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) word |= (unsigned)(src[(size_t)r * W] == 1) << r;
    bits[((size_t)p * WPC + yw) * W + x] = word;
}

// grid (min(ceil(WPC * W / 256), 64), P): the words of one object are strided over its workgroups
__global__ __launch_bounds__(256) void pr_iou_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b, int H, int W, int WPC,
                                                     int* __restrict__ counts) {
    __shared__ int part[2][4];
    const int p = blockIdx.y, n = WPC * W;
    const unsigned* __restrict__ pa = a + (size_t)p * n;
    const unsigned* __restrict__ pb = b + (size_t)p * n;
    const int last0 = (WPC - 1) * W;                                   // first word of the last word row
    const unsigned tm = tail_mask(H, WPC - 1);
    int ov = 0, un = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned m = i >= last0 ? tm : 0xffffffffu;
        const unsigned wa = pa[i] & m, wb = pb[i] & m;
        ov += __popc(wa & wb);
        un += __popc(wa | wb);
    }
    ov = wave_add(ov);
    un = wave_add(un);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = ov; part[1][wave] = un; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ov = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        un = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (ov) atomicAdd(&counts[2 * p], ov);
        if (un) atomicAdd(&counts[2 * p + 1], un);
    }
}

__global__ __launch_bounds__(256) void pr_zero_counts_kernel(int P, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * P) counts[i] = 0;
}

// keep = !(iou < threshold) with iou = overlap / (union + 1e-7) in fp64: util.compute_iou followed by the walk's comparison
__global__ __launch_bounds__(256) void pr_keep_kernel(int P, const int* __restrict__ counts, double threshold, unsigned char* __restrict__ keep) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double iou = (double)counts[2 * p] / ((double)counts[2 * p + 1] + 1e-7);
    keep[p] = (iou < threshold) ? 0 : 1;
}

__global__ __launch_bounds__(256) void pr_box_init_kernel(int P, int* __restrict__ acc) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    acc[4 * p] = PR_INF; acc[4 * p + 1] = PR_INF; acc[4 * p + 2] = -1; acc[4 * p + 3] = -1;      // min x, min y, max x, max y
}

// grid (ceil(W / 256), P): one lane per column
__global__ __launch_bounds__(256) void pr_box_kernel(const unsigned* __restrict__ bits, int H, int W, int WPC, int* __restrict__ acc) {
    const int p = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    int y0 = PR_INF, y1 = -1;
    if (x < W) {
        const unsigned* __restrict__ col = bits + (size_t)p * WPC * W + x;
        for (int yw = 0; yw < WPC; ++yw) {
            const unsigned w = col[(size_t)yw * W] & tail_mask(H, yw);
            if (w) {
                if (y0 == PR_INF) y0 = yw * 32 + __ffs(w) - 1;
                y1 = yw * 32 + 31 - __clz(w);
            }
        }
    }
    const int x0 = y1 >= 0 ? x : PR_INF, x1 = y1 >= 0 ? x : -1;
    const int my0 = wave_min(y0), my1 = wave_max(y1), mx0 = wave_min(x0), mx1 = wave_max(x1);
    if ((threadIdx.x & 63) == 0 && my1 >= 0) {
        atomicMin(&acc[4 * p], mx0); atomicMin(&acc[4 * p + 1], my0);
        atomicMax(&acc[4 * p + 2], mx1); atomicMax(&acc[4 * p + 3], my1);
    }
}

// _compute_box_from_mask -> _process_box -> ResizeLongestSide.apply_boxes -> float32, four numbers per object in fp64.  Products and
// sums stay separate roundings, as in numpy (no contraction into fused multiply-adds)
__global__ __launch_bounds__(256) void pr_box_finish_kernel(int P, int H, int W, double ext, double sx, double sy, int* acc,
                                                            unsigned char* __restrict__ nonempty) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int ix0 = acc[4 * p], iy0 = acc[4 * p + 1], ix1 = acc[4 * p + 2], iy1 = acc[4 * p + 3];
    float* out = (float*)acc + 4 * p;                                  // the same words as acc[4 p ..]: neither pointer is restrict
    if (ix1 < 0) {
        out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; out[3] = 0.f;
        nonempty[p] = 0;
        return;
    }
    const double x0 = (double)ix0, y0 = (double)iy0, x1 = (double)(ix1 + 1), y1 = (double)(iy1 + 1);      // half-open
    double ex = 0.0, ey = 0.0;
    if (ext >= 1.0) { ex = ext; ey = ext; }
    else if (ext != 0.0) { ey = ext * (y1 - y0); ex = ext * (x1 - x0); }
    const double bx0 = fmax(x0 - ex, 0.0), by0 = fmax(y0 - ey, 0.0), bx1 = fmin(x1 + ex, (double)W), by1 = fmin(y1 + ey, (double)H);
    out[0] = (float)(rint(bx0) * sx); out[1] = (float)(rint(by0) * sy);
    out[2] = (float)(rint(bx1) * sx); out[3] = (float)(rint(by1) * sy);
    nonempty[p] = 1;
}

// taps of output pixel i of the antialiased triangle filter (ATen _compute_indices_min_size_weights_aa, bilinear, align_corners = False):
// centre (i + 0.5) scale, support max(scale, 1), taps [lo, hi), weight of tap j = 1 - |j + 0.5 - centre| / support (before normalisation)
struct Taps { double centre; float inv; int lo, hi; };

MSAM_DEVINL Taps pr_taps(int i, double scale, int n_in) {
    Taps t;
    const double support = scale >= 1.0 ? scale : 1.0;
    t.centre = ((double)i + 0.5) * scale;
    t.inv = (float)(1.0 / support);
    const int lo = (int)(t.centre - support + 0.5), hi = (int)(t.centre + support + 0.5);
    t.lo = lo < 0 ? 0 : lo;
    t.hi = hi > n_in ? n_in : hi;
    return t;
}

MSAM_DEVINL float pr_weight(const Taps& t, int j) {
    const float d = fabsf((float)((double)j + 0.5 - t.centre)) * t.inv;
    return d < 1.f ? 1.f - d : 0.f;
}

// grid (PR_SIDE / PR_BAND, P), 256 threads: thread = output column, workgroup = a band of PR_BAND output rows
__global__ __launch_bounds__(256) void pr_logits_kernel(const unsigned* __restrict__ bits, int H, int W, int WPC, int th, int tw,
                                                        double scale_y, double scale_x, float hi_logit, float lo_logit,
                                                        float* __restrict__ logits) {
    const int p = blockIdx.y, oy0 = blockIdx.x * PR_BAND, ox = threadIdx.x;
    float* __restrict__ out = logits + ((size_t)p * PR_SIDE + oy0) * PR_SIDE + ox;
    if (ox >= tw || oy0 >= th) {                                       // padding of the square
#pragma unroll
        for (int k = 0; k < PR_BAND; ++k) out[(size_t)k * PR_SIDE] = lo_logit;
        return;
    }
    const Taps tx = pr_taps(ox, scale_x, W);
    float wsum_x = 0.f;
    for (int j = tx.lo; j < tx.hi; ++j) wsum_x += pr_weight(tx, j);
    Taps ty[PR_BAND];
    float acc[PR_BAND], wsum_y[PR_BAND];
    int ylo = PR_INF, yhi = 0;
#pragma unroll
    for (int k = 0; k < PR_BAND; ++k) {
        ty[k] = pr_taps(oy0 + k, scale_y, H);
        if (oy0 + k >= th) ty[k].hi = ty[k].lo;                        // a padded row: no taps
        acc[k] = 0.f; wsum_y[k] = 0.f;
        if (ty[k].lo < ty[k].hi) { ylo = ty[k].lo < ylo ? ty[k].lo : ylo; yhi = ty[k].hi > yhi ? ty[k].hi : yhi; }
    }
    const unsigned* __restrict__ base = bits + (size_t)p * WPC * W;
    for (int yw = ylo >> 5; yw * 32 < yhi; ++yw) {
        // horizontal pass for the 32 source rows of this word row: row sums in registers
        float h[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) h[r] = 0.f;
        const unsigned* __restrict__ row = base + (size_t)yw * W;
        for (int j = tx.lo; j < tx.hi; ++j) {
            const unsigned w = row[j];
            const float wt = pr_weight(tx, j);
#pragma unroll
            for (int r = 0; r < 32; ++r) h[r] += ((w >> r) & 1u) ? wt : 0.f;
        }
        // vertical pass: rows outside [lo, hi) of an output row (the rows >= H among them) take no part
#pragma unroll
        for (int k = 0; k < PR_BAND; ++k) {
            if (ty[k].hi <= yw * 32 || ty[k].lo >= yw * 32 + 32) continue;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int ys = yw * 32 + r;
                const float wt = (ys >= ty[k].lo && ys < ty[k].hi) ? pr_weight(ty[k], ys) : 0.f;
                acc[k] += wt * h[r];
                wsum_y[k] += wt;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PR_BAND; ++k) {
        const float den = wsum_x * wsum_y[k];
        const float v = den > 0.f ? acc[k] / den : 0.f;
        out[(size_t)k * PR_SIDE] = v > 0.5f ? hi_logit : lo_logit;
    }
}

// grid (ceil(W / 256) * WPC, 1): one lane per (word row, column), all objects
__global__ __launch_bounds__(256) void pr_paint_kernel(const unsigned* __restrict__ bits, const int* __restrict__ ids,
                                                       const unsigned char* __restrict__ keep, int P, int H, int W, int WPC, int XB,
                                                       int* __restrict__ label) {
    const int yw = blockIdx.x / XB, x = (blockIdx.x - yw * XB) * 256 + threadIdx.x;
    if (x >= W) return;
    int m[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) m[r] = 0;
    const unsigned tm = tail_mask(H, yw);
    unsigned any = 0;
    for (int p = 0; p < P; ++p) {
        if (keep && !keep[p]) continue;
        const unsigned w = bits[((size_t)p * WPC + yw) * W + x] & tm;
        if (!w) continue;
        const int id = ids[p];
        any |= w;
#pragma unroll
        for (int r = 0; r < 32; ++r) m[r] = ((w >> r) & 1u) && id > m[r] ? id : m[r];
    }
    if (!any) return;
    int* __restrict__ dst = label + (size_t)yw * 32 * W + x;
#pragma unroll
    for (int r = 0; r < 32; ++r)
        if ((any >> r) & 1u) {
            const int old = dst[(size_t)r * W];
            if (m[r] > old) dst[(size_t)r * W] = m[r];
        }
}

bool pr_shape_ok(int32_t P, int32_t H, int32_t W) {
    return P >= 1 && P <= MSAM_MASK_MAX_OBJECTS && H >= 1 && W >= 1 && H <= MSAM_MASK_MAX_SIDE && W <= MSAM_MASK_MAX_SIDE;
}

#define PR_SHAPE_MSG ": 1 <= P <= 65535 and 1 <= H, W <= 32767"

}  // namespace

extern "C" int msam_mask_pack(const uint8_t* masks, int32_t P, int32_t H, int32_t W, uint32_t* bits, void* stream) {
    if (!masks || !bits) { msam_set_error("msam_mask_pack: null pointer"); return 1; }
    if (!pr_shape_ok(P, H, W)) { msam_set_error("msam_mask_pack" PR_SHAPE_MSG); return 1; }
    const int WPC = (H + 31) / 32, XB = (W + 255) / 256;
    hipLaunchKernelGGL(pr_pack_kernel, dim3((unsigned)(XB * WPC), (unsigned)P), dim3(256), 0, (hipStream_t)stream, masks, H, W, WPC, XB, bits);
    return msam_check_launch("msam_mask_pack");
}

extern "C" int msam_mask_iou_counts(const uint32_t* a, const uint32_t* b, int32_t P, int32_t H, int32_t W, double threshold,
                                    int32_t* counts, uint8_t* keep, void* stream) {
    if (!a || !b || !counts || !keep) { msam_set_error("msam_mask_iou_counts: null pointer"); return 1; }
    if (!pr_shape_ok(P, H, W)) { msam_set_error("msam_mask_iou_counts" PR_SHAPE_MSG); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const int WPC = (H + 31) / 32;
    const int64_t blocks = ((int64_t)WPC * W + 255) / 256;
    hipLaunchKernelGGL(pr_zero_counts_kernel, dim3((unsigned)((2 * P + 255) / 256)), dim3(256), 0, s, P, counts);
    hipLaunchKernelGGL(pr_iou_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), (unsigned)P), dim3(256), 0, s, a, b, H, W, WPC, counts);
    hipLaunchKernelGGL(pr_keep_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, (const int*)counts, threshold, keep);
    return msam_check_launch("msam_mask_iou_counts");
}

extern "C" int msam_mask_box_prompts(const uint32_t* bits, int32_t P, int32_t H, int32_t W, double box_extension, int32_t input_h,
                                     int32_t input_w, float* boxes, uint8_t* nonempty, void* stream) {
    if (!bits || !boxes || !nonempty) { msam_set_error("msam_mask_box_prompts: null pointer"); return 1; }
    if (!pr_shape_ok(P, H, W)) { msam_set_error("msam_mask_box_prompts" PR_SHAPE_MSG); return 1; }
    if (!(box_extension >= 0.0) || !(box_extension <= 1e9)) { msam_set_error("msam_mask_box_prompts: 0 <= box_extension <= 1e9"); return 1; }
    if (input_h < 1 || input_w < 1) { msam_set_error("msam_mask_box_prompts: the input size must be positive"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const int WPC = (H + 31) / 32;
    const unsigned pb = (unsigned)((P + 255) / 256);
    int* acc = (int*)boxes;                                            // the output doubles as the integer accumulator
    hipLaunchKernelGGL(pr_box_init_kernel, dim3(pb), dim3(256), 0, s, P, acc);
    hipLaunchKernelGGL(pr_box_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)P), dim3(256), 0, s, bits, H, W, WPC, acc);
    hipLaunchKernelGGL(pr_box_finish_kernel, dim3(pb), dim3(256), 0, s, P, H, W, box_extension, (double)input_w / (double)W,
                       (double)input_h / (double)H, acc, nonempty);
    return msam_check_launch("msam_mask_box_prompts");
}

extern "C" int msam_mask_logits(const uint32_t* bits, int32_t P, int32_t H, int32_t W, float* logits, void* stream) {
    if (!bits || !logits) { msam_set_error("msam_mask_logits: null pointer"); return 1; }
    if (!pr_shape_ok(P, H, W)) { msam_set_error("msam_mask_logits" PR_SHAPE_MSG); return 1; }
    // ResizeLongestSide.get_preprocess_shape(H, W, 256), in the same fp64 arithmetic
    const double scale = PR_SIDE * 1.0 / (double)(H > W ? H : W);
    const int th = (int)((double)H * scale + 0.5), tw = (int)((double)W * scale + 0.5);
    if (th < 1 || tw < 1 || th > PR_SIDE || tw > PR_SIDE) { msam_set_error("msam_mask_logits: the resized mask has an empty side"); return 1; }
    const double eps = 1e-3;
    const float hi = (float)std::log((1 - eps) / eps), lo = (float)std::log(eps / (1 - eps));
    const int WPC = (H + 31) / 32;
    hipLaunchKernelGGL(pr_logits_kernel, dim3((unsigned)(PR_SIDE / PR_BAND), (unsigned)P), dim3(256), 0, (hipStream_t)stream, bits, H, W, WPC,
                       th, tw, (double)H / (double)th, (double)W / (double)tw, hi, lo, logits);
    return msam_check_launch("msam_mask_logits");
}

extern "C" int msam_paint_max(const uint32_t* bits, const int32_t* ids, const uint8_t* keep, int32_t P, int32_t H, int32_t W,
                              int32_t* label, void* stream) {
    if (!bits || !ids || !label) { msam_set_error("msam_paint_max: null pointer"); return 1; }
    if (!pr_shape_ok(P, H, W)) { msam_set_error("msam_paint_max" PR_SHAPE_MSG); return 1; }
    const int WPC = (H + 31) / 32, XB = (W + 255) / 256;
    hipLaunchKernelGGL(pr_paint_kernel, dim3((unsigned)(XB * WPC)), dim3(256), 0, (hipStream_t)stream, bits, ids, keep, P, H, W, WPC, XB, label);
    return msam_check_launch("msam_paint_max");
}
