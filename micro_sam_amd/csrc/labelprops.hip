// Device side of the prompt-based evaluation (micro_sam/evaluation/inference.py -> util.get_centers_and_bounding_boxes, util.py:1283-1331):
// the exact squared Euclidean distance transform and the per-object properties of a label image - area, bounding box, coordinate sums
// and the "v" centre (the object's pixel furthest from any object boundary).  Integer work throughout: every result is exact and does
// not depend on the order of the atomics.
//
//   column : g(y, x) = vertical distance to the nearest zero pixel of the column (EDT_GINF when the column has none), two sweeps per
//            column cut into segments of 32 rows so that a 1024-row image gives every CU work: the first / last zero pixel per
//            (segment, column), one short serial pass over the segments of a column for the distances carried in from above and
//            below, then one thread per (segment, column) sweeps down and up.  The zero pixels are those of a mask, or - for the label
//            properties - the INNER BOUNDARIES of the label image: label != 0 and a 4-neighbour with another label (outside the image
//            = label 0), computed on the fly.
//   row    : one workgroup per 256 pixels of a row: d2(y, x) = min over x' of (x - x')^2 + g(y, x')^2.  g(y, x)^2 is an upper bound, so
//            only |x - x'| < sqrt(best so far) can improve it: the scan walks outwards from x and stops there.  The row segment and
//            256 pixels on either side are staged in LDS; a scan that has to go further continues in global memory.
//   stats  : one thread per 8 consecutive pixels of a row: label -> index in the sorted ids (binary search), runs of one object are
//            pre-summed, then integer atomics per run: area, bounding box (min / max), coordinate sums (64-bit adds), and the maximum
//            of d2 per object.
//   centre : per pixel that reaches its object's maximum: atomicMin of the raster index - ties go to the first pixel in raster order.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

typedef unsigned long long u64;
constexpr int EDT_GINF = 65535;                                        // "no zero in this column"; real distances are <= 32766
constexpr unsigned EDT_INF = 0x7fffffffu;                              // INT32_MAX: no zero pixel anywhere
constexpr int EDT_TILE = 256, EDT_HALO = 256;
constexpr int EDT_SEG = 32;                                           // rows per thread of the column pass
constexpr int LP_PER = 8;
constexpr int LP_NONE = 0x7fffffff;

enum { SRC_U8 = 0, SRC_I32 = 1, SRC_LABELS = 2 };

// is pixel (y, x) a zero pixel of the distance transform?
template <int SRC>
MSAM_DEVINL bool edt_is_zero(const void* __restrict__ src, int H, int W, int y, int x) {
    const size_t p = (size_t)y * W + x;
    if (SRC == SRC_U8) return ((const unsigned char*)src)[p] == 0;
    if (SRC == SRC_I32) return ((const int*)src)[p] == 0;
    const int* __restrict__ lab = (const int*)src;
    const int c = lab[p];
    if (c == 0) return false;
    const int up = y > 0 ? lab[p - W] : 0, down = y + 1 < H ? lab[p + W] : 0;
    const int left = x > 0 ? lab[p - 1] : 0, right = x + 1 < W ? lab[p + 1] : 0;
    return up != c || down != c || left != c || right != c;
}

// first / last zero pixel of every (segment of EDT_SEG rows, column): top = rows from the segment's first row down to its first zero
// pixel, bot = rows from its last zero pixel down to the segment's last row; EDT_GINF when the segment has none
template <int SRC>
__global__ __launch_bounds__(64) void edt_segment_kernel(const void* __restrict__ src, int H, int W, int* __restrict__ top, int* __restrict__ bot) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int s = blockIdx.y, y0 = s * EDT_SEG, y1 = y0 + EDT_SEG < H ? y0 + EDT_SEG : H;
    int first = EDT_GINF, last = EDT_GINF;
#pragma unroll 4
    for (int y = y0; y < y1; ++y)
        if (edt_is_zero<SRC>(src, H, W, y, x)) {
            if (first == EDT_GINF) first = y - y0;
            last = y1 - 1 - y;
        }
    top[(size_t)s * W + x] = first;
    bot[(size_t)s * W + x] = last;
}

// per column, over the S segments: above[s] = distance from the segment's first row to the nearest zero pixel above the segment,
// and (written over bot) below[s] = distance from its last row to the nearest zero pixel below it
__global__ __launch_bounds__(64) void edt_carry_kernel(int H, int W, int S, const int* __restrict__ top, int* __restrict__ bot,
                                                       int* __restrict__ above) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    int c = EDT_GINF;
    for (int s = 0; s < S; ++s) {
        const int len = (s + 1) * EDT_SEG <= H ? EDT_SEG : H - s * EDT_SEG;
        const int b = bot[(size_t)s * W + x];
        above[(size_t)s * W + x] = c;
        c = b != EDT_GINF ? b + 1 : (c == EDT_GINF ? EDT_GINF : c + len);
    }
    c = EDT_GINF;
    for (int s = S - 1; s >= 0; --s) {
        const int len = (s + 1) * EDT_SEG <= H ? EDT_SEG : H - s * EDT_SEG;
        const int t = top[(size_t)s * W + x];
        bot[(size_t)s * W + x] = c;
        c = t != EDT_GINF ? t + 1 : (c == EDT_GINF ? EDT_GINF : c + len);
    }
}

// one thread per (segment, column): the two sweeps of the column pass inside the segment, started from the distances carried in
template <int SRC>
__global__ __launch_bounds__(64) void edt_column_kernel(const void* __restrict__ src, int H, int W, const int* __restrict__ above,
                                                        const int* __restrict__ below, int* __restrict__ g) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int s = blockIdx.y, y0 = s * EDT_SEG, y1 = y0 + EDT_SEG < H ? y0 + EDT_SEG : H;
    int cur = above[(size_t)s * W + x];
    if (cur != EDT_GINF) --cur;                                        // (the value of the row above the segment)
#pragma unroll 4
    for (int y = y0; y < y1; ++y) {
        cur = edt_is_zero<SRC>(src, H, W, y, x) ? 0 : (cur == EDT_GINF ? EDT_GINF : cur + 1);
        g[(size_t)y * W + x] = cur;
    }
    cur = below[(size_t)s * W + x];
    if (cur != EDT_GINF) --cur;
#pragma unroll 4
    for (int y = y1 - 1; y >= y0; --y) {
        const int v = g[(size_t)y * W + x];
        cur = v == 0 ? 0 : (cur == EDT_GINF ? EDT_GINF : cur + 1);
        if (cur < v) g[(size_t)y * W + x] = cur;
    }
}

MSAM_DEVINL unsigned edt_take(unsigned best, int dx, int a, int b) {
    const int m = a < b ? a : b;                                       // (EDT_GINF is the largest value)
    if (m == EDT_GINF) return best;
    const unsigned cand = (unsigned)(dx * dx) + (unsigned)(m * m);     // <= 2 * 32766^2 < 2^31
    return cand < best ? cand : best;
}

// FG_ONLY: pixels whose label is 0 get 0 (the label properties never read them)
template <bool FG_ONLY>
__global__ __launch_bounds__(256) void edt_row_kernel(const int* __restrict__ g, const int* __restrict__ labels, int W, int* __restrict__ out) {
    __shared__ int sg[EDT_TILE + 2 * EDT_HALO];
    const int y = blockIdx.y, x0 = blockIdx.x * EDT_TILE;
    const int* __restrict__ grow = g + (size_t)y * W;
    for (int i = threadIdx.x; i < EDT_TILE + 2 * EDT_HALO; i += 256) {
        const int xs = x0 - EDT_HALO + i;
        sg[i] = (xs >= 0 && xs < W) ? grow[xs] : EDT_GINF;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    const size_t p = (size_t)y * W + x;
    if (FG_ONLY && labels[p] == 0) { out[p] = 0; return; }
    const int c = EDT_HALO + threadIdx.x;
    const int gc = sg[c];
    unsigned best = gc == EDT_GINF ? EDT_INF : (unsigned)(gc * gc);
    const int reach = x > W - 1 - x ? x : W - 1 - x;                    // furthest column of the row
    int dx = 1;
    for (; dx <= EDT_HALO && dx <= reach && (unsigned)(dx * dx) < best; ++dx) best = edt_take(best, dx, sg[c - dx], sg[c + dx]);
    for (; dx <= reach && (unsigned)(dx * dx) < best; ++dx)            // beyond the staged part of the row
        best = edt_take(best, dx, x - dx >= 0 ? grow[x - dx] : EDT_GINF, x + dx < W ? grow[x + dx] : EDT_GINF);
    out[p] = (int)best;
}

MSAM_DEVINL int lp_find(const int* __restrict__ ids, int n, int v) {   // index of v in ids[0, n), -1 if absent
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && ids[lo] == v) ? lo : -1;
}

__global__ __launch_bounds__(256) void lp_check_ids_kernel(const int* __restrict__ ids, int n, int* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (ids[i] <= 0 || (i > 0 && ids[i - 1] >= ids[i])) atomicExch(flag, 1);
}

__global__ __launch_bounds__(256) void lp_init_kernel(int n, int* __restrict__ area, int* __restrict__ bbox, u64* __restrict__ sums,
                                                      int* __restrict__ maxd, int* __restrict__ first) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    area[o] = 0;
    bbox[4 * o] = LP_NONE; bbox[4 * o + 1] = LP_NONE; bbox[4 * o + 2] = 0; bbox[4 * o + 3] = 0;
    sums[2 * o] = 0; sums[2 * o + 1] = 0;
    maxd[o] = -1; first[o] = LP_NONE;
}

// dist == nullptr: no centres wanted (index and maxd are not written)
__global__ __launch_bounds__(256) void lp_stats_kernel(const int* __restrict__ labels, const int* __restrict__ dist, int W,
                                                       const int* __restrict__ ids, int n, int* __restrict__ index, int* __restrict__ area,
                                                       int* __restrict__ bbox, u64* __restrict__ sums, int* __restrict__ maxd) {
    const int y = blockIdx.y;
    const int xb = (blockIdx.x * 256 + threadIdx.x) * LP_PER;
    if (xb >= W) return;
    const size_t row = (size_t)y * W;
    auto flush = [&](int o, int xa, int cnt, int md) {
        if (o < 0) return;
        atomicAdd(&area[o], cnt);
        atomicMin(&bbox[4 * o], y); atomicMin(&bbox[4 * o + 1], xa);
        atomicMax(&bbox[4 * o + 2], y + 1); atomicMax(&bbox[4 * o + 3], xa + cnt);
        atomicAdd(&sums[2 * o], (u64)cnt * (u64)y);
        atomicAdd(&sums[2 * o + 1], (u64)cnt * (u64)xa + (u64)cnt * (u64)(cnt - 1) / 2);
        if (dist) atomicMax(&maxd[o], md);
    };
    int prev_lab = 0, prev_o = -1, run_o = -1, run_x = 0, run_n = 0, run_d = 0;
    const int xe = xb + LP_PER < W ? xb + LP_PER : W;
    for (int x = xb; x < xe; ++x) {
        const int lab = labels[row + x];
        const int o = lab == prev_lab ? prev_o : (lab > 0 ? lp_find(ids, n, lab) : -1);
        prev_lab = lab; prev_o = o;
        const int d = (dist && o >= 0) ? dist[row + x] : 0;
        if (dist) index[row + x] = o;
        if (o == run_o) { ++run_n; run_d = d > run_d ? d : run_d; }
        else { flush(run_o, run_x, run_n, run_d); run_o = o; run_x = x; run_n = 1; run_d = d; }
    }
    flush(run_o, run_x, run_n, run_d);
}

__global__ __launch_bounds__(256) void lp_center_kernel(const int* __restrict__ index, const int* __restrict__ dist, int npx,
                                                        const int* __restrict__ maxd, int* __restrict__ first) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const int o = index[p];
    if (o >= 0 && dist[p] == maxd[o]) atomicMin(&first[o], p);
}

__global__ __launch_bounds__(256) void lp_finish_kernel(int n, int W, const int* __restrict__ area, int* __restrict__ bbox,
                                                        const int* __restrict__ first, int* __restrict__ center) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    if (area[o] == 0) {                                                // an id the image does not hold
        bbox[4 * o] = 0; bbox[4 * o + 1] = 0;
        if (center) { center[2 * o] = -1; center[2 * o + 1] = -1; }
        return;
    }
    if (center) { const int p = first[o]; center[2 * o] = p / W; center[2 * o + 1] = p - (p / W) * W; }
}

bool lp_side_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && H <= MSAM_EDT_MAX_SIDE && W <= MSAM_EDT_MAX_SIDE; }

int64_t edt_carry_ints(int H, int W) { return (int64_t)((H + EDT_SEG - 1) / EDT_SEG) * W * 3; }   // top, bot / below, above per (segment, column)

template <int SRC>
void edt_launch(const void* src, const int* labels, int H, int W, int* g, int* carry, int* out, hipStream_t s) {
    const int S = (H + EDT_SEG - 1) / EDT_SEG;
    int* top = carry;
    int* bot = top + (size_t)S * W;
    int* above = bot + (size_t)S * W;
    const dim3 cols((unsigned)((W + 63) / 64), (unsigned)S);
    hipLaunchKernelGGL((edt_segment_kernel<SRC>), cols, dim3(64), 0, s, src, H, W, top, bot);
    hipLaunchKernelGGL(edt_carry_kernel, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, H, W, S, (const int*)top, bot, above);
    hipLaunchKernelGGL((edt_column_kernel<SRC>), cols, dim3(64), 0, s, src, H, W, (const int*)above, (const int*)bot, g);
    const dim3 grid((unsigned)((W + EDT_TILE - 1) / EDT_TILE), (unsigned)H);
    if (SRC == SRC_LABELS) hipLaunchKernelGGL((edt_row_kernel<true>), grid, dim3(256), 0, s, (const int*)g, labels, W, out);
    else hipLaunchKernelGGL((edt_row_kernel<false>), grid, dim3(256), 0, s, (const int*)g, labels, W, out);
}

}  // namespace

extern "C" int64_t msam_edt_squared_workspace_bytes(int32_t H, int32_t W) {
    return lp_side_ok(H, W) ? ((int64_t)H * W + edt_carry_ints(H, W)) * 4 : 0;
}

extern "C" int msam_edt_squared(const void* mask, int32_t mask_is_int32, int32_t H, int32_t W, int32_t* out, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    if (!mask || !out || !workspace) { msam_set_error("msam_edt_squared: null pointer"); return 1; }
    if (!lp_side_ok(H, W)) { msam_set_error("msam_edt_squared: 1 <= H, W <= 32767"); return 1; }
    if (mask_is_int32 != 0 && mask_is_int32 != 1) { msam_set_error("msam_edt_squared: mask_is_int32 must be 0 (uint8) or 1 (int32)"); return 1; }
    if (workspace_bytes < msam_edt_squared_workspace_bytes(H, W)) {
        msam_set_error("msam_edt_squared: the workspace is smaller than msam_edt_squared_workspace_bytes says");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    int* g = (int*)workspace;
    if (mask_is_int32) edt_launch<SRC_I32>(mask, nullptr, H, W, g, g + (size_t)H * W, out, s);
    else edt_launch<SRC_U8>(mask, nullptr, H, W, g, g + (size_t)H * W, out, s);
    return msam_check_launch("msam_edt_squared");
}

extern "C" int64_t msam_label_props_workspace_bytes(int32_t H, int32_t W, int32_t N) {
    if (!lp_side_ok(H, W) || N < 1) return 0;
    // g, d2, object index per pixel; maximum and first pixel per object; flag; the column pass's carries
    return (int64_t)H * W * 12 + (int64_t)N * 8 + 16 + edt_carry_ints(H, W) * 4;
}

extern "C" int msam_label_props(const int32_t* labels, int32_t H, int32_t W, const int32_t* ids, int32_t N, int32_t* area, int32_t* bbox,
                                int64_t* coord_sum, int32_t* center, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!labels || !ids || !area || !bbox || !coord_sum || !workspace) { msam_set_error("msam_label_props: null pointer"); return 1; }
    if (!lp_side_ok(H, W)) { msam_set_error("msam_label_props: 1 <= H, W <= 32767"); return 1; }
    if (N < 1) { msam_set_error("msam_label_props: N >= 1 ids"); return 1; }
    if (workspace_bytes < msam_label_props_workspace_bytes(H, W, N)) {
        msam_set_error("msam_label_props: the workspace is smaller than msam_label_props_workspace_bytes says");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;
    int* g = (int*)workspace;
    int* dist = g + npx;
    int* index = dist + npx;
    int* maxd = index + npx;
    int* first = maxd + N;
    int* flag = first + N;
    int* carry = flag + 4;
    // the ids are the caller's and on the device: they are checked there, and the answer is awaited before anything is written
    int bad = 0;
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) { msam_set_error("msam_label_props: memset failed"); return 2; }
    hipLaunchKernelGGL(lp_check_ids_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, ids, N, flag);
    if (hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        msam_set_error("msam_label_props: reading the id check failed");
        return 2;
    }
    if (bad) { msam_set_error("msam_label_props: ids must be positive, distinct and sorted ascending"); return 1; }
    const unsigned nb = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(lp_init_kernel, dim3(nb), dim3(256), 0, s, N, area, bbox, (u64*)coord_sum, maxd, first);
    if (center) edt_launch<SRC_LABELS>(labels, labels, H, W, g, carry, dist, s);
    const dim3 grid((unsigned)((W + 256 * LP_PER - 1) / (256 * LP_PER)), (unsigned)H);
    hipLaunchKernelGGL(lp_stats_kernel, grid, dim3(256), 0, s, labels, center ? (const int*)dist : (const int*)nullptr, W, ids, N, index, area,
                       bbox, (u64*)coord_sum, maxd);
    if (center)
        hipLaunchKernelGGL(lp_center_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, (const int*)index, (const int*)dist, (int)npx,
                           (const int*)maxd, first);
    hipLaunchKernelGGL(lp_finish_kernel, dim3(nb), dim3(256), 0, s, N, W, (const int*)area, bbox, (const int*)first, center);
    return msam_check_launch("msam_label_props");
}
