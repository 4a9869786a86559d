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
//
// msam_distance_targets (the training targets of torch_em's PerObjectDistanceTransform, restated in DESIGN.md section 8.4) turns the same
// passes towards labels 1..N: the zero pixels are scikit-image's find_boundaries(mode="inner") - only neighbours INSIDE the image count -,
// the object index is the label itself, and one pixel-parallel pass writes the foreground, centre-distance and boundary-distance planes
// from a 16-byte record per object.
//
// msam_seed_centers (the first stage of AutomaticPromptGenerator.generate: _derive_point_prompts -> _get_centers, reference
// micro_sam/instance_segmentation.py:1322-1379) runs from the three decoder maps to one point per seed component without a host pass:
//   seeds    : (c < ct) && (b < bt) && !(f < ft) per pixel, compared in fp64
//   label    : msam_label_components_async (segment.hip): per pixel the block-major key of its component's first pixel
//   interior : one byte per pixel, 0 on the zero set Z = find_boundaries(mode="outer") of the component image (+ the image border)
//   rank     : the roots in ascending key order get 1..N (per 4096 keys: count, one scan of the counts, ballot ranks)
//   column   : the passes above on `interior`, with a carry pass that starts anew in every row of 512 x 512 blocks and looks 16 rows
//              beyond it - elf.parallel.distance_transform(halo=(16, 16), block_shape=(512, 512)) computes every block on its own
//   row      : as above inside the block's 16-column halo, on component pixels only; one 64-bit atomic maximum per pixel of
//              (d2 << 32 | ~raster index) selects the largest distance and, among equals, the first pixel in raster order
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

enum { SRC_U8 = 0, SRC_I32 = 1, SRC_LABELS = 2, SRC_INNER = 3 };

// labels 1..n are objects; every other value (0, negative, above n) is background and is never used as an index
MSAM_DEVINL bool lp_is_object(int lab, int n) { return (unsigned)(lab - 1) < (unsigned)n; }

// is pixel (y, x) a zero pixel of the distance transform?  nmax: the largest object label (SRC_INNER only)
template <int SRC>
MSAM_DEVINL bool edt_is_zero(const void* __restrict__ src, int H, int W, int nmax, int y, int x) {
    const size_t p = (size_t)y * W + x;
    if (SRC == SRC_U8) return ((const unsigned char*)src)[p] == 0;
    if (SRC == SRC_I32) return ((const int*)src)[p] == 0;
    const int* __restrict__ lab = (const int*)src;
    const int c = lab[p];
    if (SRC == SRC_INNER) {                                            // an object pixel with another value next to it INSIDE the image
        if (!lp_is_object(c, nmax)) return false;
        auto differs = [&](int v) { return (lp_is_object(v, nmax) ? v : 0) != c; };
        return (y > 0 && differs(lab[p - W])) || (y + 1 < H && differs(lab[p + W])) || (x > 0 && differs(lab[p - 1])) ||
               (x + 1 < W && differs(lab[p + 1]));
    }
    if (c == 0) return false;
    const int up = y > 0 ? lab[p - W] : 0, down = y + 1 < H ? lab[p + W] : 0;
    const int left = x > 0 ? lab[p - 1] : 0, right = x + 1 < W ? lab[p + 1] : 0;
    return up != c || down != c || left != c || right != c;
}

// first / last zero pixel of every (segment of EDT_SEG rows, column): top = rows from the segment's first row down to its first zero
// pixel, bot = rows from its last zero pixel down to the segment's last row; EDT_GINF when the segment has none
template <int SRC>
__global__ __launch_bounds__(64) void edt_segment_kernel(const void* __restrict__ src, int H, int W, int nmax, int* __restrict__ top,
                                                         int* __restrict__ bot) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int s = blockIdx.y, y0 = s * EDT_SEG, y1 = y0 + EDT_SEG < H ? y0 + EDT_SEG : H;
    int first = EDT_GINF, last = EDT_GINF;
#pragma unroll 4
    for (int y = y0; y < y1; ++y)
        if (edt_is_zero<SRC>(src, H, W, nmax, y, x)) {
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
__global__ __launch_bounds__(64) void edt_column_kernel(const void* __restrict__ src, int H, int W, int nmax, const int* __restrict__ above,
                                                        const int* __restrict__ below, int* __restrict__ g) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int s = blockIdx.y, y0 = s * EDT_SEG, y1 = y0 + EDT_SEG < H ? y0 + EDT_SEG : H;
    int cur = above[(size_t)s * W + x];
    if (cur != EDT_GINF) --cur;                                        // (the value of the row above the segment)
#pragma unroll 4
    for (int y = y0; y < y1; ++y) {
        cur = edt_is_zero<SRC>(src, H, W, nmax, y, x) ? 0 : (cur == EDT_GINF ? EDT_GINF : cur + 1);
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

// SKIP = 1: pixels whose label is 0 get 0 (the label properties never read them); SKIP = 2: every pixel that is no object 1..nmax
template <int SKIP>
__global__ __launch_bounds__(256) void edt_row_kernel(const int* __restrict__ g, const int* __restrict__ labels, int W, int nmax,
                                                      int* __restrict__ out) {
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
    if (SKIP == 1 && labels[p] == 0) { out[p] = 0; return; }
    if (SKIP == 2 && !lp_is_object(labels[p], nmax)) { out[p] = 0; return; }
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

// dist == nullptr: no centres wanted (index and maxd are not written).  CONSEC: the objects are the labels 1..n themselves (object index =
// label - 1; ids and index are not used)
template <bool CONSEC>
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
        const int o = CONSEC ? (lp_is_object(lab, n) ? lab - 1 : -1) : (lab == prev_lab ? prev_o : (lab > 0 ? lp_find(ids, n, lab) : -1));
        prev_lab = lab; prev_o = o;
        const int d = (dist && o >= 0) ? dist[row + x] : 0;
        if (!CONSEC && dist) index[row + x] = o;
        if (o == run_o) { ++run_n; run_d = d > run_d ? d : run_d; }
        else { flush(run_o, run_x, run_n, run_d); run_o = o; run_x = x; run_n = 1; run_d = d; }
    }
    flush(run_o, run_x, run_n, run_d);
}

// CONSEC: index is the label image itself and n the largest label
template <bool CONSEC>
__global__ __launch_bounds__(256) void lp_center_kernel(const int* __restrict__ index, const int* __restrict__ dist, int npx, int n,
                                                        const int* __restrict__ maxd, int* __restrict__ first) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const int o = CONSEC ? (lp_is_object(index[p], n) ? index[p] - 1 : -1) : index[p];
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
void edt_launch(const void* src, const int* labels, int H, int W, int nmax, int* g, int* carry, int* out, hipStream_t s) {
    const int S = (H + EDT_SEG - 1) / EDT_SEG;
    int* top = carry;
    int* bot = top + (size_t)S * W;
    int* above = bot + (size_t)S * W;
    const dim3 cols((unsigned)((W + 63) / 64), (unsigned)S);
    hipLaunchKernelGGL((edt_segment_kernel<SRC>), cols, dim3(64), 0, s, src, H, W, nmax, top, bot);
    hipLaunchKernelGGL(edt_carry_kernel, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, H, W, S, (const int*)top, bot, above);
    hipLaunchKernelGGL((edt_column_kernel<SRC>), cols, dim3(64), 0, s, src, H, W, nmax, (const int*)above, (const int*)bot, g);
    const dim3 grid((unsigned)((W + EDT_TILE - 1) / EDT_TILE), (unsigned)H);
    if (SRC == SRC_INNER) hipLaunchKernelGGL((edt_row_kernel<2>), grid, dim3(256), 0, s, (const int*)g, labels, W, nmax, out);
    else if (SRC == SRC_LABELS) hipLaunchKernelGGL((edt_row_kernel<1>), grid, dim3(256), 0, s, (const int*)g, labels, W, nmax, out);
    else hipLaunchKernelGGL((edt_row_kernel<0>), grid, dim3(256), 0, s, (const int*)g, labels, W, nmax, out);
}

// ---- msam_distance_targets: what the final pass reads per object
struct __attribute__((aligned(16))) DtObject {
    int cy, cx;                                                        // the centre
    float bden, cden;                                                  // denominators of the boundary and the centre channel
};

constexpr int DT_PER = 4;                                              // pixels per thread of the vector form of the final pass

MSAM_DEVINL int dt_round_half_even(u64 s, u64 a) {                     // s / a rounded half to even, exactly
    const u64 q = s / a, r = s - q * a;
    if (2 * r < a) return (int)q;
    if (2 * r > a) return (int)q + 1;
    return (int)(q + (q & 1));
}

// The normalisation of the centre channel - the ONE place that fixes it.  torch_em divides the distances to the centre by their maximum
// over the object's bounding-box CROP, taken before the crop is masked to the object; the distance to a point is convex, so that maximum
// lies on one of the crop's four corner pixels: R^2 = max(cy - y0, y1 - 1 - cy)^2 + max(cx - x0, x1 - 1 - cx)^2.
MSAM_DEVINL int dt_center_norm2(int cy, int cx, int y0, int x0, int y1, int x1) {
    const int dy = cy - y0 > y1 - 1 - cy ? cy - y0 : y1 - 1 - cy;
    const int dx = cx - x0 > x1 - 1 - cx ? cx - x0 : x1 - 1 - cx;
    return dy * dy + dx * dx;                                          // <= 2 * 32766^2 < 2^31
}

__global__ __launch_bounds__(256) void dt_finish_kernel(const int* __restrict__ labels, int W, int n, int correct, const int* __restrict__ area,
                                                        const u64* __restrict__ sums, const int* __restrict__ maxd, const int* __restrict__ first,
                                                        int* __restrict__ bbox, int* __restrict__ center, int* __restrict__ dmax2,
                                                        DtObject* __restrict__ table) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    DtObject t;
    if (area[o] == 0) {                                                // a label the image does not hold (the final pass never reads its record)
        bbox[4 * o] = 0; bbox[4 * o + 1] = 0;
        center[2 * o] = -1; center[2 * o + 1] = -1; dmax2[o] = 0;
        t.cy = -1; t.cx = -1; t.bden = INFINITY; t.cden = INFINITY;
        table[o] = t;
        return;
    }
    const u64 a = (u64)area[o];
    int cy = dt_round_half_even(sums[2 * o], a), cx = dt_round_half_even(sums[2 * o + 1], a);
    if (correct && labels[(size_t)cy * W + cx] != o + 1) {             // the centroid lies outside: the first pixel of maximal distance
        const int p = first[o];
        cy = p / W; cx = p - cy * W;
    }
    // an image without any boundary pixel (EDT_INF everywhere) holds one object: its boundary channel is 1
    const int dm = (unsigned)maxd[o] == EDT_INF ? 0 : maxd[o];
    center[2 * o] = cy; center[2 * o + 1] = cx; dmax2[o] = dm;
    t.cy = cy; t.cx = cx;
    t.bden = dm == 0 ? INFINITY : sqrtf((float)dm) + 1e-7f;            // d2 / inf = 0: the channel is 1 on such an object
    t.cden = sqrtf((float)dt_center_norm2(cy, cx, bbox[4 * o], bbox[4 * o + 1], bbox[4 * o + 2], bbox[4 * o + 3])) + 1e-7f;
    table[o] = t;
}

// V pixels per thread, consecutive in raster order (V = 4: 16-byte loads and stores; npx is then a multiple of 4 and every plane 16-byte
// aligned).  table == nullptr: no objects, d2 is not read
template <int V>
__global__ __launch_bounds__(256) void dt_write_kernel(const int* __restrict__ labels, const int* __restrict__ d2, unsigned npx, unsigned W, int n,
                                                       const DtObject* __restrict__ table, float fill, float* __restrict__ out) {
    const unsigned p0 = (blockIdx.x * 256u + threadIdx.x) * V;
    if (p0 >= npx) return;
    int lab[V], dd[V];
    float fg[V], ce[V], bd[V];
    if (V == 4) {
        const uint4 l = *(const uint4*)(labels + p0);
        lab[0] = (int)l.x; lab[1] = (int)l.y; lab[2] = (int)l.z; lab[3] = (int)l.w;
        if (table) { const uint4 d = *(const uint4*)(d2 + p0); dd[0] = (int)d.x; dd[1] = (int)d.y; dd[2] = (int)d.z; dd[3] = (int)d.w; }
    } else {
        lab[0] = labels[p0];
        if (table) dd[0] = d2[p0];
    }
    unsigned y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        fg[i] = 0.f; ce[i] = fill; bd[i] = fill;
        if (table && lp_is_object(lab[i], n)) {
            const DtObject t = table[lab[i] - 1];
            const int dy = (int)y - t.cy, dx = (int)x - t.cx;
            fg[i] = 1.f;
            ce[i] = sqrtf((float)(dy * dy + dx * dx)) / t.cden;
            bd[i] = 1.f - sqrtf((float)dd[i]) / t.bden;
        }
        if (++x == W) { x = 0; ++y; }
    }
    if (V == 4) {
        *(float4*)(out + p0) = make_float4(fg[0], fg[1], fg[2], fg[3]);
        *(float4*)(out + (size_t)npx + p0) = make_float4(ce[0], ce[1], ce[2], ce[3]);
        *(float4*)(out + 2 * (size_t)npx + p0) = make_float4(bd[0], bd[1], bd[2], bd[3]);
    } else {
        out[p0] = fg[0]; out[(size_t)npx + p0] = ce[0]; out[2 * (size_t)npx + p0] = bd[0];
    }
}

int64_t dt_pixel_bytes(int H, int W) { return ((int64_t)H * W * 8 + 15) / 16 * 16; }   // g and d2, rounded up so that the records stay aligned

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
    if (mask_is_int32) edt_launch<SRC_I32>(mask, nullptr, H, W, 0, g, g + (size_t)H * W, out, s);
    else edt_launch<SRC_U8>(mask, nullptr, H, W, 0, g, g + (size_t)H * W, out, s);
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
    if (center) edt_launch<SRC_LABELS>(labels, labels, H, W, 0, g, carry, dist, s);
    const dim3 grid((unsigned)((W + 256 * LP_PER - 1) / (256 * LP_PER)), (unsigned)H);
    hipLaunchKernelGGL((lp_stats_kernel<false>), grid, dim3(256), 0, s, labels, center ? (const int*)dist : (const int*)nullptr, W, ids, N, index, area,
                       bbox, (u64*)coord_sum, maxd);
    if (center)
        hipLaunchKernelGGL((lp_center_kernel<false>), dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, (const int*)index, (const int*)dist,
                           (int)npx, N, (const int*)maxd, first);
    hipLaunchKernelGGL(lp_finish_kernel, dim3(nb), dim3(256), 0, s, N, W, (const int*)area, bbox, (const int*)first, center);
    return msam_check_launch("msam_label_props");
}

extern "C" int64_t msam_distance_targets_workspace_bytes(int32_t H, int32_t W, int32_t N) {
    if (!lp_side_ok(H, W) || N < 0) return 0;
    // g, d2 per pixel; record (16 bytes), coordinate sums (two 64-bit words), area, maximum and first pixel per object; the column pass's carries
    return dt_pixel_bytes(H, W) + (int64_t)N * 44 + edt_carry_ints(H, W) * 4;
}

extern "C" int msam_distance_targets(const int32_t* labels, int32_t H, int32_t W, int32_t N, int32_t correct_centers, float fill, float* out,
                                     int32_t* center, int32_t* dmax2, int32_t* bbox, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!labels || !out || !workspace || (N > 0 && (!center || !dmax2 || !bbox))) { msam_set_error("msam_distance_targets: null pointer"); return 1; }
    if (!lp_side_ok(H, W)) { msam_set_error("msam_distance_targets: 1 <= H, W <= 32767"); return 1; }
    if (N < 0) { msam_set_error("msam_distance_targets: N >= 0 objects"); return 1; }
    if (correct_centers != 0 && correct_centers != 1) { msam_set_error("msam_distance_targets: correct_centers must be 0 or 1"); return 1; }
    if (((uintptr_t)workspace & 15) != 0) { msam_set_error("msam_distance_targets: the workspace must be 16-byte aligned"); return 1; }
    if (workspace_bytes < msam_distance_targets_workspace_bytes(H, W, N)) {
        msam_set_error("msam_distance_targets: the workspace is smaller than msam_distance_targets_workspace_bytes says");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;                                  // <= 32767^2 < 2^30: 32-bit pixel indices
    int* g = (int*)workspace;
    int* dist = g + npx;
    DtObject* table = (DtObject*)((char*)workspace + dt_pixel_bytes(H, W));
    u64* sums = (u64*)(table + N);
    int* area = (int*)(sums + 2 * (size_t)N);
    int* maxd = area + N;
    int* first = maxd + N;
    int* carry = first + N;
    if (N > 0) {
        const unsigned nb = (unsigned)(((int64_t)N + 255) / 256);
        hipLaunchKernelGGL(lp_init_kernel, dim3(nb), dim3(256), 0, s, N, area, bbox, sums, maxd, first);
        edt_launch<SRC_INNER>(labels, labels, H, W, N, g, carry, dist, s);
        const dim3 grid((unsigned)((W + 256 * LP_PER - 1) / (256 * LP_PER)), (unsigned)H);
        hipLaunchKernelGGL((lp_stats_kernel<true>), grid, dim3(256), 0, s, labels, (const int*)dist, W, (const int*)nullptr, N, (int*)nullptr, area,
                           bbox, sums, maxd);
        hipLaunchKernelGGL((lp_center_kernel<true>), dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, labels, (const int*)dist, (int)npx, N,
                           (const int*)maxd, first);
        hipLaunchKernelGGL(dt_finish_kernel, dim3(nb), dim3(256), 0, s, labels, W, N, correct_centers, (const int*)area, (const u64*)sums,
                           (const int*)maxd, (const int*)first, bbox, center, dmax2, table);
    }
    const DtObject* tab = N > 0 ? table : nullptr;
    const bool wide = npx % DT_PER == 0 && (((uintptr_t)labels | (uintptr_t)out) & 15) == 0;
    if (wide)
        hipLaunchKernelGGL((dt_write_kernel<DT_PER>), dim3((unsigned)((npx / DT_PER + 255) / 256)), dim3(256), 0, s, labels, (const int*)dist,
                           (unsigned)npx, (unsigned)W, N, tab, fill, out);
    else
        hipLaunchKernelGGL((dt_write_kernel<1>), dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, labels, (const int*)dist, (unsigned)npx,
                           (unsigned)W, N, tab, fill, out);
    return msam_check_launch("msam_distance_targets");
}

// ---- msam_seed_centers
namespace {

constexpr int SC_BLOCK = 512, SC_HALO = 16;                            // block_shape and halo of elf.parallel.distance_transform
constexpr int SC_KEYS = 4096;                                          // keys per workgroup of the ranking (16 rounds of 256)
static_assert(SC_BLOCK % EDT_SEG == 0 && SC_BLOCK % EDT_TILE == 0, "segments and row tiles nest inside the 512 x 512 blocks");

// NaN compares false on every side, as in numpy: a NaN foreground keeps a seed, a NaN distance drops it
__global__ __launch_bounds__(256) void sc_seed_kernel(const float* __restrict__ f, const float* __restrict__ c, const float* __restrict__ b,
                                                      int npx, double ft, double ct, double bt, int* __restrict__ seeds) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    seeds[p] = ((double)c[p] < ct && (double)b[p] < bt && !((double)f[p] < ft)) ? 1 : 0;
}

// interior[p] = 0 on the zero set Z of the distance transform, 1 elsewhere.  Z = find_boundaries(mode="outer") of the component image:
//   background pixel: an edge neighbour inside the image is an object;
//   object pixel    : scikit-image asks for an edge neighbour of another value AND a different object in the 8-neighbourhood.  The
//                     objects are the 4-connected components of a binary image, so an object edge neighbour is of the same component:
//                     a different object can only sit on a diagonal.  If the diagonal neighbour q of p is of another component, the
//                     two pixels that share an edge with both p and q (inside the image, since they lie between p and q) are
//                     background, or they would join p and q - so p has an edge neighbour of another value as well.  The rule
//                     therefore is: a diagonal neighbour inside the image belongs to another component;
//   avoid_border    : every pixel of the first and the last row and column.
__global__ __launch_bounds__(256) void sc_interior_kernel(const int* __restrict__ roots, int H, int W, int avoid_border,
                                                          unsigned char* __restrict__ interior) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t p = (size_t)y * W + x;
    const bool up = y > 0, down = y + 1 < H, left = x > 0, right = x + 1 < W;
    const int r = roots[p];
    bool zero;
    if (avoid_border && !(up && down && left && right)) zero = true;
    else if (r < 0) zero = (up && roots[p - W] >= 0) || (down && roots[p + W] >= 0) || (left && roots[p - 1] >= 0) || (right && roots[p + 1] >= 0);
    else {
        auto other = [&](int v) { return v >= 0 && v != r; };
        zero = (up && left && other(roots[p - W - 1])) || (up && right && other(roots[p - W + 1])) ||
               (down && left && other(roots[p + W - 1])) || (down && right && other(roots[p + W + 1]));
    }
    interior[p] = zero ? 0 : 1;
}

// key k is a root when the pixel it names holds k
MSAM_DEVINL bool sc_is_root(const int* __restrict__ roots, int k, int npx, int H, int W) { return k < npx && roots[bm_pix(k, H, W)] == k; }

__global__ __launch_bounds__(256) void sc_count_kernel(const int* __restrict__ roots, int H, int W, int npx, int* __restrict__ counts) {
    __shared__ int part[4];
    const int k0 = blockIdx.x * SC_KEYS + threadIdx.x;
    int cnt = 0;
    for (int i = 0; i < SC_KEYS / 256; ++i) cnt += __popcll(__ballot(sc_is_root(roots, k0 + i * 256, npx, H, W)));     // the wave's count
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one workgroup: counts -> exclusive prefix sums in place; result = {N, 0 (the "undefined" flag), (the labelling's flag: untouched), 0}
__global__ __launch_bounds__(256) void sc_scan_kernel(int* __restrict__ counts, int nblk, int* __restrict__ result) {
    __shared__ int part[256];
    const int per = (nblk + 255) / 256, i0 = threadIdx.x * per, i1 = i0 + per < nblk ? i0 + per : nblk;
    int sum = 0;
    for (int i = i0; i < i1; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        result[0] = run; result[1] = 0; result[3] = 0;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = i0; i < i1; ++i) { const int v = counts[i]; counts[i] = run; run += v; }
}

// rank[k] = 0-based rank of root key k among the roots; the records of the components below `cap` are cleared here
__global__ __launch_bounds__(256) void sc_rank_kernel(const int* __restrict__ roots, int H, int W, int npx, const int* __restrict__ offsets,
                                                      int cap, int* __restrict__ rank, u64* __restrict__ best, int* __restrict__ corner) {
    constexpr int R = SC_KEYS / 256;
    __shared__ int tot[R * 4];
    const int k0 = blockIdx.x * SC_KEYS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0;                                                  // bit i: this thread's key of round i is a root
    int before[R];                                                      // roots of the same wave and round at lower lanes
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const bool is = sc_is_root(roots, k0 + i * 256, npx, H, W);
        const u64 bal = __ballot(is);
        mine |= is ? 1u << i : 0u;
        before[i] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) tot[i * 4 + wave] = __popcll(bal);
    }
    __syncthreads();
    if (!mine) return;
    int run = offsets[blockIdx.x];
#pragma unroll
    for (int i = 0; i < R; ++i) {                                       // keys grow with (round, wave, lane)
        for (int w = 0; w < 4; ++w) {
            if (w == wave && ((mine >> i) & 1u)) {
                const int o = run + before[i];
                rank[k0 + i * 256] = o;
                if (o < cap) { best[o] = 0; corner[2 * o] = LP_NONE; corner[2 * o + 1] = LP_NONE; }
            }
            run += tot[i * 4 + w];
        }
    }
}

// the carry pass of the column sweeps, per (column, row of 512 x 512 blocks): the distances carried into the block's segments start
// from the 16 rows above and below the block and never cross them
__global__ __launch_bounds__(64) void sc_carry_kernel(const unsigned char* __restrict__ interior, int H, int W, const int* __restrict__ top,
                                                      int* __restrict__ bot, int* __restrict__ above) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int y0 = blockIdx.y * SC_BLOCK, y1 = y0 + SC_BLOCK < H ? y0 + SC_BLOCK : H;
    const int s0 = y0 / EDT_SEG, s1 = (y1 + EDT_SEG - 1) / EDT_SEG;
    int c = EDT_GINF;
    for (int d = 1; d <= SC_HALO && y0 - d >= 0; ++d)
        if (interior[(size_t)(y0 - d) * W + x] == 0) { c = d; break; }
    for (int s = s0; s < s1; ++s) {
        const int len = (s + 1) * EDT_SEG <= H ? EDT_SEG : H - s * EDT_SEG;
        const int b = bot[(size_t)s * W + x];
        above[(size_t)s * W + x] = c;
        c = b != EDT_GINF ? b + 1 : (c == EDT_GINF ? EDT_GINF : c + len);
    }
    c = EDT_GINF;
    for (int d = 0; d < SC_HALO && y1 + d < H; ++d)
        if (interior[(size_t)(y1 + d) * W + x] == 0) { c = d + 1; break; }
    for (int s = s1 - 1; s >= s0; --s) {
        const int len = (s + 1) * EDT_SEG <= H ? EDT_SEG : H - s * EDT_SEG;
        const int t = top[(size_t)s * W + x];
        bot[(size_t)s * W + x] = c;
        c = t != EDT_GINF ? t + 1 : (c == EDT_GINF ? EDT_GINF : c + len);
    }
}

// *p = max(*p, v): a compare-and-swap loop that most calls leave after the first read (the record only grows)
MSAM_DEVINL void sc_atomic_max64(u64* p, u64 v) {
    u64 old = *(volatile u64*)p;
    while (old < v) {
        const u64 seen = atomicCAS(p, old, v);
        if (seen == old) break;
        old = seen;
    }
}

// edt_row_kernel inside the window of the pixel's block (its columns grown by 16, clipped to the image), on component pixels only; the
// squared distance goes straight into the component's record.  A tile of 256 pixels lies inside one block.
__global__ __launch_bounds__(256) void sc_row_kernel(const int* __restrict__ g, const int* __restrict__ roots, const int* __restrict__ rank,
                                                     int W, int cap, u64* __restrict__ best, int* __restrict__ corner, int* __restrict__ result) {
    __shared__ int sg[EDT_TILE + 2 * EDT_HALO];
    const int y = blockIdx.y, x0 = blockIdx.x * EDT_TILE;
    const int bx0 = x0 / SC_BLOCK * SC_BLOCK;
    const int wlo = bx0 - SC_HALO > 0 ? bx0 - SC_HALO : 0, whi = bx0 + SC_BLOCK + SC_HALO < W ? bx0 + SC_BLOCK + SC_HALO : W;
    const int* __restrict__ grow = g + (size_t)y * W;
    for (int i = threadIdx.x; i < EDT_TILE + 2 * EDT_HALO; i += 256) {
        const int xs = x0 - EDT_HALO + i;
        sg[i] = (xs >= wlo && xs < whi) ? grow[xs] : EDT_GINF;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    const unsigned p = (unsigned)y * (unsigned)W + (unsigned)x;         // < 2^30
    const int r = roots[p];
    if (r < 0) return;
    const int c = EDT_HALO + threadIdx.x;
    const int gc = sg[c];
    unsigned d2 = gc == EDT_GINF ? EDT_INF : (unsigned)(gc * gc);
    const int reach = x - wlo > whi - 1 - x ? x - wlo : whi - 1 - x;    // furthest column of the window
    int dx = 1;
    for (; dx <= EDT_HALO && dx <= reach && (unsigned)(dx * dx) < d2; ++dx) d2 = edt_take(d2, dx, sg[c - dx], sg[c + dx]);
    for (; dx <= reach && (unsigned)(dx * dx) < d2; ++dx)               // beyond the staged part of the row
        d2 = edt_take(d2, dx, x - dx >= wlo ? grow[x - dx] : EDT_GINF, x + dx < whi ? grow[x + dx] : EDT_GINF);
    if (d2 == EDT_INF) atomicExch(&result[1], 1);                       // no pixel of Z in the window: the reference's value is undefined
    const int o = rank[r];
    if (o >= cap) return;
    sc_atomic_max64(&best[o], ((u64)d2 << 32) | (u64)(0xffffffffu - p));
    if (d2 == 0) { atomicMin(&corner[2 * o], y); atomicMin(&corner[2 * o + 1], x); }    // read only when every pixel of o holds 0
}

__global__ __launch_bounds__(256) void sc_finish_kernel(const int* __restrict__ result, int cap, int W, const u64* __restrict__ best,
                                                        const int* __restrict__ corner, int* __restrict__ centers) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= cap || o >= result[0]) return;
    const u64 b = best[o];
    if ((b >> 32) == 0) {                                               // argmax of an all-zero crop: the corner of the bounding box
        centers[2 * o] = corner[2 * o]; centers[2 * o + 1] = corner[2 * o + 1];
    } else {
        const unsigned p = 0xffffffffu - (unsigned)(b & 0xffffffffull);
        centers[2 * o] = (int)(p / (unsigned)W); centers[2 * o + 1] = (int)(p % (unsigned)W);
    }
}

int64_t sc_blocks(int H, int W) { return ((int64_t)H * W + SC_KEYS - 1) / SC_KEYS; }

}  // namespace

// segment.hip's.  A weak reference: this file still links on its own (the host build of the tests compiles it alone), and
// msam_seed_centers refuses where the labelling is absent.
extern "C" __attribute__((weak)) int msam_label_components_async(const int32_t* seg, int32_t H, int32_t W, int32_t* roots, int32_t* changed_flag,
                                                                 int32_t passes, void* stream);

extern "C" int64_t msam_seed_centers_workspace_bytes(int32_t H, int32_t W, int32_t max_centers) {
    if (!lp_side_ok(H, W) || max_centers < 1) return 0;
    // record (64-bit) and corner (two words) per component; seeds / rank, roots, g per pixel; the column pass's carries; the ranking's counts;
    // one byte per pixel
    return (int64_t)max_centers * 16 + (int64_t)H * W * 12 + edt_carry_ints(H, W) * 4 + sc_blocks(H, W) * 4 + (int64_t)H * W;
}

extern "C" int msam_seed_centers(const float* foreground, const float* center_distances, const float* boundary_distances, int32_t H, int32_t W,
                                 double foreground_threshold, double center_distance_threshold, double boundary_distance_threshold,
                                 int32_t avoid_image_border, int32_t* centers, int32_t max_centers, int32_t* result, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (!foreground || !center_distances || !boundary_distances || !centers || !result || !workspace) {
        msam_set_error("msam_seed_centers: null pointer");
        return 1;
    }
    if (!lp_side_ok(H, W)) { msam_set_error("msam_seed_centers: 1 <= H, W <= 32767"); return 1; }
    if (max_centers < 1) { msam_set_error("msam_seed_centers: max_centers >= 1"); return 1; }
    if (foreground_threshold != foreground_threshold || center_distance_threshold != center_distance_threshold ||
        boundary_distance_threshold != boundary_distance_threshold) {
        msam_set_error("msam_seed_centers: a threshold is NaN");
        return 1;
    }
    if (avoid_image_border != 0 && avoid_image_border != 1) { msam_set_error("msam_seed_centers: avoid_image_border must be 0 or 1"); return 1; }
    if (((uintptr_t)workspace & 7) != 0) { msam_set_error("msam_seed_centers: the workspace must be 8-byte aligned"); return 1; }
    if (workspace_bytes < msam_seed_centers_workspace_bytes(H, W, max_centers)) {
        msam_set_error("msam_seed_centers: the workspace is smaller than msam_seed_centers_workspace_bytes says");
        return 1;
    }
    if (!msam_label_components_async) { msam_set_error("msam_seed_centers: this build lacks msam_label_components_async (segment.hip)"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const size_t npx = (size_t)H * W;                                  // <= 32767^2 < 2^30: 32-bit pixel indices and keys
    const int nblk = (int)sc_blocks(H, W);
    u64* best = (u64*)workspace;
    int* corner = (int*)(best + max_centers);
    int* seeds = corner + 2 * (size_t)max_centers;                     // the rank per root key once the labelling has read the seeds
    int* roots = seeds + npx;
    int* g = roots + npx;
    int* carry = g + npx;
    int* counts = carry + edt_carry_ints(H, W);
    unsigned char* interior = (unsigned char*)(counts + nblk);
    const unsigned pb = (unsigned)((npx + 255) / 256);
    hipLaunchKernelGGL(sc_seed_kernel, dim3(pb), dim3(256), 0, s, foreground, center_distances, boundary_distances, (int)npx, foreground_threshold,
                       center_distance_threshold, boundary_distance_threshold, seeds);
    const int e = msam_label_components_async(seeds, H, W, roots, result + 2, 1, s);     // result[2]: 0 = the labelling is complete
    if (e) return e;
    hipLaunchKernelGGL(sc_interior_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H), dim3(256), 0, s, (const int*)roots, H, W,
                       avoid_image_border, interior);
    hipLaunchKernelGGL(sc_count_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const int*)roots, H, W, (int)npx, counts);
    hipLaunchKernelGGL(sc_scan_kernel, dim3(1), dim3(256), 0, s, counts, nblk, result);
    int* rank = seeds;
    hipLaunchKernelGGL(sc_rank_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const int*)roots, H, W, (int)npx, (const int*)counts, max_centers,
                       rank, best, corner);
    const int S = (H + EDT_SEG - 1) / EDT_SEG;
    int* top = carry;
    int* bot = top + (size_t)S * W;
    int* above = bot + (size_t)S * W;
    const dim3 cols((unsigned)((W + 63) / 64), (unsigned)S);
    hipLaunchKernelGGL((edt_segment_kernel<SRC_U8>), cols, dim3(64), 0, s, (const void*)interior, H, W, 0, top, bot);
    hipLaunchKernelGGL(sc_carry_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + SC_BLOCK - 1) / SC_BLOCK)), dim3(64), 0, s,
                       (const unsigned char*)interior, H, W, (const int*)top, bot, above);
    hipLaunchKernelGGL((edt_column_kernel<SRC_U8>), cols, dim3(64), 0, s, (const void*)interior, H, W, 0, (const int*)above, (const int*)bot, g);
    hipLaunchKernelGGL(sc_row_kernel, dim3((unsigned)((W + EDT_TILE - 1) / EDT_TILE), (unsigned)H), dim3(256), 0, s, (const int*)g,
                       (const int*)roots, (const int*)rank, W, max_centers, best, corner, result);
    hipLaunchKernelGGL(sc_finish_kernel, dim3((unsigned)(((int64_t)max_centers + 255) / 256)), dim3(256), 0, s, (const int*)result, max_centers, W,
                       (const u64*)best, (const int*)corner, centers);
    return msam_check_launch("msam_seed_centers");
}
