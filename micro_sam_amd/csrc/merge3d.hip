// Device side of merging per-slice instance segmentations across z (multi_dimensional_segmentation.merge_instance_segmentation_3d;
// reference micro_sam/multi_dimensional_segmentation.py:236-309, :312-382): everything around the multicut that walks the whole label
// volume - the gap closing of _preprocess_closing, the per-id slice ranges behind the uniqueness check and _filter_z_extent, and the
// lookup of the cluster labels.  The overlap table is csrc/segment.hip's msam_slice_overlaps; the multicut stays on the host.
//
//   close gaps : labels int32 [Z, H, W] -> out, integer for integer the host's _preprocess_closing.  Only the ORDER of
//                the numbers the host paints matters, so no component number is materialised:
//                  closed   per pixel column, closed[z] = AND_{|c - z| <= gap} OR_{|s - c| <= gap, s in the volume} (labels[s] > 0);
//                  label    8-connected components of closed[z] for all interior slices in one batch, union-find on LINEAR pixel
//                           indices (the smallest index is the root = the component's first pixel in raster order = skimage's number
//                           order; the block-major keys of segment.hip differ from it beyond 512 columns): 64 x 32 tiles in LDS, the
//                           edges across tile borders on the global array, one compression with the edge check.  All 4-edges are
//                           united; a diagonal edge only where both pixels at its other two corners are background (otherwise the two
//                           4-edges through that corner join its ends already);
//                  stats    per root the smallest and the largest label of slice z under the component (atomic min / max): the
//                           component is KEPT when it holds at most one distinct label;
//                  mark     one bit per (slice, id): on an edge slice the ids that occur, on an interior slice the set I = ids that
//                           occur inside a component that is not kept;
//                  survive  a kept root survives when one of its pixels is not painted over by a label of I;
//                  ranks    surviving kept roots by pixel index (block counts, a scan, ranks inside a block), ids by their bit position
//                           (word prefix sums), the running offset of the slices by one thread over Z counts;
//                  paint    a pixel whose label is marked: offset + kept roots + rank of the label; else inside a kept component:
//                           offset + rank of the root; else 0.
//   z ranges   : zr[id] = (first slice, last slice) an id occurs in, atomic min / max.
//   lut        : out[p] = lut[labels[p]].
//
// Integer atomics only, and only min / max / or, whose result does not depend on their order: two calls agree bit for bit.  The
// workspace is the caller's; kernels on the caller's stream, no allocation, no synchronisation.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int MG_TW = 64, MG_TH = 32, MG_ROWS = MG_TH / 4;          // a tile is one wave wide, a wave owns 8 of its rows
constexpr int MG_PER = 16, MG_CHUNK = 256 * MG_PER;                   // pixels per thread / per workgroup of the rank kernels
constexpr int MG_NONE = 0x7fffffff;

MSAM_DEVINL bool mg_fg(int v, int lim) { return v > 0 && v < lim; }   // (a label outside [0, lim) is flagged by the paint kernel and reads as 0)
MSAM_DEVINL bool mg_edge_slice(int z, int Z, int g) { return z < g || z >= Z - g; }

// closed[z] of pixel column p, z an interior slice (every c below lies inside the volume)
MSAM_DEVINL int mg_closed(const int* __restrict__ labels, long HW, long p, int z, int Z, int g, int lim) {
    if (mg_fg(labels[(long)z * HW + p], lim)) return 1;               // closed >= foreground
    for (int c = z - g; c <= z + g; ++c) {
        bool any = false;
        const int s1 = min(c + g, Z - 1);
        for (int s = max(c - g, 0); s <= s1 && !any; ++s) any = mg_fg(labels[(long)s * HW + p], lim);
        if (!any) return 0;
    }
    return 1;
}

MSAM_DEVINL int mg_find(const int* par, int i) {                      // root of the tree node i is in (par[i] >= 0)
    int r = par[i];
    while (true) { const int p = par[r]; if (p == r) break; r = p; }
    return r;
}

// lock-free union, the smaller index becomes the root (csrc/segment.hip cc_border_kernel: why no link is lost)
MSAM_DEVINL void mg_union(int* par, int i, int j) {
    int a = mg_find(par, i), b = mg_find(par, j);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) break;
        a = old;
    }
}

// exclusive prefix sum of one value per thread over the 256 threads of the workgroup; every thread calls it
MSAM_DEVINL int mg_block_scan(int v, int* sh, int* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

// ---- level 1: one workgroup per (interior slice, tile).  L[zi][p] = linear index of the tile-local root, -1 where closed is 0.
__global__ __launch_bounds__(256) void mg_tile_kernel(const int* __restrict__ labels, int Z, int H, int W, int g, int lim, int tilesX,
                                                      int tilesY, int* __restrict__ L) {
    __shared__ int par[MG_TW * MG_TH];
    __shared__ unsigned char cls[(MG_TH + 1) * MG_TW];
    int b = blockIdx.x;
    const int tx = b % tilesX; b /= tilesX;
    const int ty = b % tilesY, zi = b / tilesY;
    const long HW = (long)H * W;
    const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * MG_ROWS;
    const int tx0 = tx * MG_TW, ty0 = ty * MG_TH, gx = tx0 + lane;
    int c[MG_ROWS + 1];
#pragma unroll
    for (int k = 0; k < MG_ROWS; ++k) {
        const int gy = ty0 + r0 + k;
        c[k] = (gx < W && gy < H) ? mg_closed(labels, HW, (long)gy * W + gx, zi + g, Z, g, lim) : 0;
        cls[(r0 + k) * MG_TW + lane] = (unsigned char)c[k];
    }
    if (threadIdx.x < MG_TW) cls[MG_TH * MG_TW + threadIdx.x] = 0;       // the row below the tile: another tile's
    __syncthreads();
    c[MG_ROWS] = cls[(r0 + MG_ROWS) * MG_TW + lane];
    unsigned vert = 0u, dlm = 0u, drm = 0u;                              // bit k: row k's edge to the pixel below / below left / below right
#pragma unroll
    for (int k = 0; k < MG_ROWS; ++k) {
        const int l_ = __shfl(c[k], (lane + 63) & 63), r_ = __shfl(c[k], (lane + 1) & 63);
        const int dl_ = __shfl(c[k + 1], (lane + 63) & 63), dr_ = __shfl(c[k + 1], (lane + 1) & 63);
        const bool left = lane > 0 && l_ != 0, right = lane < 63 && r_ != 0;
        const bool dl = lane > 0 && dl_ != 0, dr = lane < 63 && dr_ != 0;
        const bool cont = left && c[k] != 0;                             // continues the run of the pixel to the left
        const unsigned long long starts = __ballot(c[k] != 0 && !cont);
        const unsigned long long upto = starts & ((2ull << lane) - 1ull);     // (lane 63: 2 << 63 wraps to 0, mask = all ones)
        const uint32_t hi = (uint32_t)(upto >> 32);
        const int start = hi ? 63 - __clz(hi) : 31 - __clz((uint32_t)upto);   // last run start at or before this lane
        par[(r0 + k) * MG_TW + lane] = c[k] != 0 ? (r0 + k) * MG_TW + start : -1;
        if (c[k] != 0) {
            if (c[k + 1] != 0) { if (!(cont && dl)) vert |= 1u << k; }       // (else the left neighbour's edge joins the same two runs)
            else {
                if (dl && !left) dlm |= 1u << k;
                if (dr && !right) drm |= 1u << k;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MG_ROWS; ++k) {
        const int i = (r0 + k) * MG_TW + lane;
        if ((vert >> k) & 1u) mg_union(par, i, i + MG_TW);
        if ((dlm >> k) & 1u) mg_union(par, i, i + MG_TW - 1);
        if ((drm >> k) & 1u) mg_union(par, i, i + MG_TW + 1);
    }
    __syncthreads();
    int* __restrict__ Ls = L + (long)zi * HW;
#pragma unroll
    for (int k = 0; k < MG_ROWS; ++k) {
        const int gy = ty0 + r0 + k;
        if (gx >= W || gy >= H) continue;
        int key = -1;
        if (c[k] != 0) {
            const int r = mg_find(par, (r0 + k) * MG_TW + lane);
            key = (ty0 + r / MG_TW) * W + tx0 + (r % MG_TW);
        }
        Ls[(long)gy * W + gx] = key;
    }
}

// ---- level 2: one thread per pixel of the last column / last row of a tile that has a neighbour tile: the edges across the border
__global__ __launch_bounds__(256) void mg_border_kernel(int H, int W, int nvx, int nhy, int bps, int* L) {
    const int zi = blockIdx.x / bps;
    const long t = (long)(blockIdx.x - zi * bps) * 256 + threadIdx.x;
    int* Ls = L + (long)zi * H * W;
    const long nv = (long)nvx * H;
    auto on = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W && Ls[y * W + x] >= 0; };
    if (t < nv) {                                          // right border of tile column c: x = c * MG_TW + MG_TW - 1, x + 1 < W
        const int c = (int)(t / H), y = (int)(t - (long)c * H), x = c * MG_TW + MG_TW - 1;
        if (!on(y, x)) return;
        const int i = y * W + x;
        if (on(y, x + 1)) {
            if (!((y % MG_TH) != 0 && on(y - 1, x) && on(y - 1, x + 1))) mg_union(Ls, i, i + 1);
        } else {
            if (on(y + 1, x + 1) && !on(y + 1, x)) mg_union(Ls, i, i + W + 1);
            if (on(y - 1, x + 1) && !on(y - 1, x)) mg_union(Ls, i, i - W + 1);
        }
    } else {                                               // lower border of tile row r: y = r * MG_TH + MG_TH - 1, y + 1 < H
        const long u = t - nv;
        if (u >= (long)nhy * W) return;
        const int r = (int)(u / W), x = (int)(u - (long)r * W), y = r * MG_TH + MG_TH - 1;
        if (!on(y, x)) return;
        const int i = y * W + x;
        if (on(y + 1, x)) {
            if (!((x % MG_TW) != 0 && on(y, x - 1) && on(y + 1, x - 1))) mg_union(Ls, i, i + W);
        } else {
            if (on(y + 1, x - 1) && !on(y, x - 1)) mg_union(Ls, i, i + W - 1);
            if (on(y + 1, x + 1) && !on(y, x + 1)) mg_union(Ls, i, i + W + 1);
        }
    }
}

// ---- compression + check (the runtime witness of the labelling: `incomplete` is set when two 8-neighbours end in different roots); a
// root's label statistics are initialised here
__global__ __launch_bounds__(256) void mg_compress_kernel(int H, int W, long n, int* L, int* __restrict__ cmin, int* __restrict__ cmax,
                                                          int* __restrict__ incomplete) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long HW = (long)H * W;
    const long zi = i / HW;
    const int p = (int)(i - zi * HW);
    int* Ls = L + zi * HW;
    const int raw = Ls[p];
    if (raw < 0) return;
    int r = raw;
    while (true) { const int q = Ls[r]; if (q == r) break; r = q; }
    if (r != raw) Ls[p] = r;
    if (r == p) { cmin[i] = MG_NONE; cmax[i] = 0; }
    const int y = p / W, x = p - y * W;
    bool bad = false;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int dy = d == 0 ? 0 : 1, dx = d == 0 ? 1 : d - 2;        // right, below left, below, below right
        if (y + dy >= H || x + dx < 0 || x + dx >= W) continue;
        const int j = (y + dy) * W + x + dx;
        const int q = Ls[j];
        if (q < 0 || q == raw || q == r) continue;                      // (an entry is at any time one of the pixel's ancestors)
        bad = bad || mg_find(Ls, j) != r;
    }
    if (bad) *incomplete = 1;
}

// ---- smallest / largest label of the slice under every component.  A pixel whose left neighbour has the same label leaves the update to it.
__global__ __launch_bounds__(256) void mg_stats_kernel(const int* __restrict__ labels, int H, int W, int g, int lim, long n,
                                                       const int* __restrict__ L, int* __restrict__ cmin, int* __restrict__ cmax) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long HW = (long)H * W;
    const long zi = i / HW;
    const int p = (int)(i - zi * HW);
    const int* __restrict__ lab = labels + (zi + g) * HW;
    const int v = lab[p];
    if (!mg_fg(v, lim)) return;
    if ((p % W) != 0 && lab[p - 1] == v) return;
    const int r = L[i];
    if (r < 0) return;                                                  // (cannot happen: closed >= foreground)
    atomicMin(&cmin[zi * HW + r], v);
    atomicMax(&cmax[zi * HW + r], v);
}

// ---- one bit per (slice, id): the ids of an edge slice; on an interior slice the ids inside a component with two or more labels
__global__ __launch_bounds__(256) void mg_mark_kernel(const int* __restrict__ labels, int Z, int H, int W, int g, int lim, int words,
                                                      const int* __restrict__ L, const int* __restrict__ cmin,
                                                      const int* __restrict__ cmax, unsigned* __restrict__ bits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long HW = (long)H * W;
    if (i >= (long)Z * HW) return;
    const int z = (int)(i / HW);
    const int p = (int)(i - (long)z * HW);
    const int v = labels[i];
    if (!mg_fg(v, lim)) return;
    if ((p % W) != 0 && labels[i - 1] == v) return;
    if (!mg_edge_slice(z, Z, g)) {
        const long base = (long)(z - g) * HW;
        const int r = L[base + p];
        if (r < 0 || cmin[base + r] == cmax[base + r]) return;
    }
    atomicOr(&bits[(long)z * words + (v >> 5)], 1u << (v & 31));
}

// ---- a root's statistics become its state: cmax = 0 kept, -1 not kept
__global__ __launch_bounds__(256) void mg_rootstate_kernel(long HW, long n, const int* __restrict__ L, const int* __restrict__ cmin,
                                                           int* __restrict__ cmax) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (L[i] != (int)(i % HW)) return;
    const int hi = cmax[i];
    cmax[i] = (hi == 0 || cmin[i] == hi) ? 0 : -1;
}

// ---- a kept root with a pixel that no marked label paints over survives: cmax = 1 (every writer stores the same value)
__global__ __launch_bounds__(256) void mg_survive_kernel(const int* __restrict__ labels, long HW, int g, int lim, int words, long n,
                                                         const int* __restrict__ L, int* cmax, const unsigned* __restrict__ bits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = L[i];
    if (r < 0) return;
    const long zi = i / HW;
    const long ci = zi * HW + r;
    if (cmax[ci] != 0) return;                                           // not kept, or known to survive
    const int v = labels[i + (long)g * HW];
    if (mg_fg(v, lim) && ((bits[(zi + g) * words + (v >> 5)] >> (v & 31)) & 1u)) return;
    cmax[ci] = 1;
}

MSAM_DEVINL bool mg_surviving_root(const int* __restrict__ Ls, const int* __restrict__ cs, long HW, int p) {
    return p < HW && Ls[p] == p && cs[p] == 1;
}

// ---- surviving roots per chunk of MG_CHUNK pixels
__global__ __launch_bounds__(256) void mg_count_kernel(long HW, int nb, const int* __restrict__ L, const int* __restrict__ cmax,
                                                       int* __restrict__ bcnt) {
    __shared__ int sh[256];
    const int zi = blockIdx.x / nb, blk = blockIdx.x - zi * nb;
    const int* __restrict__ Ls = L + (long)zi * HW;
    const int* __restrict__ cs = cmax + (long)zi * HW;
    int cnt = 0;
    for (int k = 0; k < MG_PER; ++k) {
        const long p = (long)blk * MG_CHUNK + threadIdx.x * MG_PER + k;
        cnt += (p < HW && mg_surviving_root(Ls, cs, HW, (int)p)) ? 1 : 0;
    }
    int total;
    mg_block_scan(cnt, sh, &total);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = total;
}

// ---- per slice: prefix sums over the words of its bit row (wpre, nids) and, on an interior slice, over its chunk counts (in place, nkept)
__global__ __launch_bounds__(256) void mg_scan_kernel(int Z, int g, int words, int nb, const unsigned* __restrict__ bits,
                                                      int* __restrict__ wpre, int* __restrict__ nids, int* __restrict__ bcnt,
                                                      int* __restrict__ nkept) {
    __shared__ int sh[256];
    const int z = blockIdx.x, t = threadIdx.x;
    int carry = 0, total;
    for (int base = 0; base < words; base += 256) {
        const bool in = base + t < words;
        const int c = in ? __popc(bits[(long)z * words + base + t]) : 0;
        const int ex = mg_block_scan(c, sh, &total);
        if (in) wpre[(long)z * words + base + t] = carry + ex;
        carry += total;
    }
    if (t == 0) nids[z] = carry;
    carry = 0;
    if (!mg_edge_slice(z, Z, g)) {
        int* __restrict__ row = bcnt + (long)(z - g) * nb;
        for (int base = 0; base < nb; base += 256) {
            const bool in = base + t < nb;
            const int c = in ? row[base + t] : 0;
            const int ex = mg_block_scan(c, sh, &total);
            if (in) row[base + t] = carry + ex;
            carry += total;
        }
    }
    if (t == 0) nkept[z] = carry;
}

// ---- the running offset of the host loop: Z small counts, one thread.  Edge slice: offset += n, back to 1 when the slice is empty (the
// reference's own line, offset = max + 1); interior slice: offset += n.
__global__ void mg_offset_kernel(int Z, int g, const int* __restrict__ nids, const int* __restrict__ nkept, int* __restrict__ off,
                                 int* __restrict__ result) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int offset = 1;
    for (int z = 0; z < Z; ++z) {
        off[z] = offset;
        const int n = nids[z] + nkept[z];
        if (n > 0) offset += n;
        else if (mg_edge_slice(z, Z, g)) offset = 1;
    }
    result[0] = offset;
}

// ---- rank of every surviving root among those of its slice, by pixel index: written over its cmin
__global__ __launch_bounds__(256) void mg_rank_kernel(long HW, int nb, const int* __restrict__ L, const int* __restrict__ cmax,
                                                      const int* __restrict__ bcnt, int* __restrict__ cmin) {
    __shared__ int sh[256];
    const int zi = blockIdx.x / nb, blk = blockIdx.x - zi * nb;
    const int* __restrict__ Ls = L + (long)zi * HW;
    const int* __restrict__ cs = cmax + (long)zi * HW;
    unsigned flags = 0u;
    for (int k = 0; k < MG_PER; ++k) {
        const long p = (long)blk * MG_CHUNK + threadIdx.x * MG_PER + k;
        if (p < HW && mg_surviving_root(Ls, cs, HW, (int)p)) flags |= 1u << k;
    }
    int total;
    int rank = bcnt[blockIdx.x] + mg_block_scan(__popc(flags), sh, &total);
    for (int k = 0; k < MG_PER; ++k)
        if ((flags >> k) & 1u) cmin[(long)zi * HW + (long)blk * MG_CHUNK + threadIdx.x * MG_PER + k] = rank++;
}

// ---- every pixel takes its value; a label outside [0, lim) is reported (1: negative, 2: >= lim) and reads as 0
__global__ __launch_bounds__(256) void mg_paint_kernel(const int* __restrict__ labels, int Z, int H, int W, int g, int lim, int words,
                                                       const int* __restrict__ L, const int* __restrict__ cmin,
                                                       const int* __restrict__ cmax, const unsigned* __restrict__ bits,
                                                       const int* __restrict__ wpre, const int* __restrict__ nkept,
                                                       const int* __restrict__ off, int* __restrict__ out, int* __restrict__ result) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long HW = (long)H * W;
    if (i >= (long)Z * HW) return;
    const int z = (int)(i / HW);
    const int v = labels[i];
    if (v < 0) atomicOr(&result[1], 1);
    else if (v >= lim) atomicOr(&result[1], 2);
    int val = 0;
    if (mg_fg(v, lim)) {
        const long w = (long)z * words + (v >> 5);
        const unsigned word = bits[w];
        if ((word >> (v & 31)) & 1u) val = off[z] + nkept[z] + wpre[w] + __popc(word & ((1u << (v & 31)) - 1u));
    }
    if (val == 0 && !mg_edge_slice(z, Z, g)) {
        const long base = (long)(z - g) * HW;
        const int r = L[base + (i - (long)z * HW)];
        if (r >= 0 && cmax[base + r] >= 0) val = off[z] + cmin[base + r];
    }
    out[i] = val;
}

// ---- z ranges
__global__ __launch_bounds__(256) void mg_zr_init_kernel(int n_ids, int Z, int* __restrict__ zr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_ids) { zr[2 * i] = Z; zr[2 * i + 1] = -1; }
}

__global__ __launch_bounds__(256) void mg_zr_kernel(const int* __restrict__ labels, int Z, int W, long HW, int n_ids, int* __restrict__ zr,
                                                    int* __restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Z * HW) return;
    const int v = labels[i];
    if (v == 0) return;
    if (v < 0 || v >= n_ids) { atomicOr(flag, 1); return; }
    const long p = i % HW;
    if ((p % W) != 0 && labels[i - 1] == v) return;                     // the left neighbour reports the same (id, slice)
    const int z = (int)(i / HW);
    atomicMin(&zr[2 * v], z);
    atomicMax(&zr[2 * v + 1], z);
}

// ---- lookup
__global__ __launch_bounds__(256) void mg_lut_kernel(const int* labels, long n, const int* __restrict__ lut, int n_lut, int* out,
                                                     int* __restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = labels[i];
    int o = 0;
    if (v < 0 || v >= n_lut) atomicOr(flag, 1);
    else o = lut[v];
    out[i] = o;
}

struct MgPlan {                                                          // the workspace, in int32 words
    int Zi, words, nb;
    long HW, nI;
    long o_L, o_cmin, o_cmax, o_bcnt, o_bits, o_wpre, o_nids, o_nkept, o_off, total;
};

long mg_up(long v) { return (v + 63) & ~63L; }

bool mg_plan(int32_t Z, int32_t H, int32_t W, int32_t gap, int32_t id_limit, MgPlan* pl) {
    if (Z < 1 || H < 1 || W < 1 || gap < 1 || id_limit < 1) return false;
    const long HW = (long)H * W;
    if (HW >= (1L << 31) - 2 * MG_CHUNK || (long)Z * HW >= (1L << 38)) return false;
    pl->HW = HW;
    pl->Zi = 2L * gap >= Z ? 0 : Z - 2 * gap;
    pl->words = (int)(((long)id_limit + 31) / 32);
    pl->nb = (int)((HW + MG_CHUNK - 1) / MG_CHUNK);
    pl->nI = (long)pl->Zi * HW;
    const long tiles = (long)((W + MG_TW - 1) / MG_TW) * ((H + MG_TH - 1) / MG_TH) * pl->Zi;
    if (tiles >= (1L << 31) || (long)Z * pl->words >= (1L << 34)) return false;
    long o = 0;
    pl->o_L = o; o += mg_up(pl->nI);
    pl->o_cmin = o; o += mg_up(pl->nI);
    pl->o_cmax = o; o += mg_up(pl->nI);
    pl->o_bcnt = o; o += mg_up((long)pl->Zi * pl->nb);
    pl->o_bits = o; o += mg_up((long)Z * pl->words);
    pl->o_wpre = o; o += mg_up((long)Z * pl->words);
    pl->o_nids = o; o += mg_up(Z);
    pl->o_nkept = o; o += mg_up(Z);
    pl->o_off = o; o += mg_up(Z);
    pl->total = o;
    return true;
}

#define MG_SHAPE_MSG ": Z, H, W >= 1, H * W below 2^31, Z * H * W below 2^38"

unsigned mg_blocks(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int64_t msam_close_gaps_workspace_bytes(int32_t Z, int32_t H, int32_t W, int32_t gap, int32_t id_limit) {
    MgPlan pl;
    return mg_plan(Z, H, W, gap, id_limit, &pl) ? (int64_t)pl.total * 4 : 0;
}

extern "C" int msam_close_gaps(const int32_t* labels, int32_t Z, int32_t H, int32_t W, int32_t gap, int32_t id_limit, int32_t* out,
                               int32_t* result, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!labels || !out || !result || !workspace) { msam_set_error("msam_close_gaps: null pointer"); return 1; }
    MgPlan pl;
    if (!mg_plan(Z, H, W, gap, id_limit, &pl)) {
        msam_set_error("msam_close_gaps" MG_SHAPE_MSG ", gap >= 1, id_limit >= 1 (Z * ceil(id_limit / 32) below 2^34)");
        return 1;
    }
    if (workspace_bytes < (int64_t)pl.total * 4) { msam_set_error("msam_close_gaps: the workspace is smaller than msam_close_gaps_workspace_bytes"); return 1; }
    if (((uintptr_t)workspace & 3) != 0) { msam_set_error("msam_close_gaps: the workspace must be 4-byte aligned"); return 1; }
    if (out == labels) { msam_set_error("msam_close_gaps: out must not be labels (a pixel reads the labels of other slices)"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    int* ws = (int*)workspace;
    int *L = ws + pl.o_L, *cmin = ws + pl.o_cmin, *cmax = ws + pl.o_cmax, *bcnt = ws + pl.o_bcnt, *wpre = ws + pl.o_wpre;
    int *nids = ws + pl.o_nids, *nkept = ws + pl.o_nkept, *off = ws + pl.o_off;
    unsigned* bits = (unsigned*)(ws + pl.o_bits);
    if (hipMemsetAsync(result, 0, 16, s) != hipSuccess || hipMemsetAsync(bits, 0, (size_t)Z * pl.words * 4, s) != hipSuccess) {
        msam_set_error("msam_close_gaps: memset failed");
        return 2;
    }
    const long nI = pl.nI, nA = (long)Z * pl.HW;
    if (pl.Zi > 0) {
        const int tilesX = (W + MG_TW - 1) / MG_TW, tilesY = (H + MG_TH - 1) / MG_TH;
        hipLaunchKernelGGL(mg_tile_kernel, dim3((unsigned)((long)tilesX * tilesY * pl.Zi)), dim3(256), 0, s, labels, Z, H, W, gap, id_limit,
                           tilesX, tilesY, L);
        const int nvx = (W - 1) / MG_TW, nhy = (H - 1) / MG_TH;
        const long edges = (long)nvx * H + (long)nhy * W;
        if (edges > 0) {
            const int bps = (int)((edges + 255) / 256);
            hipLaunchKernelGGL(mg_border_kernel, dim3((unsigned)((long)bps * pl.Zi)), dim3(256), 0, s, H, W, nvx, nhy, bps, L);
        }
        hipLaunchKernelGGL(mg_compress_kernel, dim3(mg_blocks(nI)), dim3(256), 0, s, H, W, nI, L, cmin, cmax, result + 2);
        hipLaunchKernelGGL(mg_stats_kernel, dim3(mg_blocks(nI)), dim3(256), 0, s, labels, H, W, gap, id_limit, nI, (const int*)L, cmin, cmax);
    }
    hipLaunchKernelGGL(mg_mark_kernel, dim3(mg_blocks(nA)), dim3(256), 0, s, labels, Z, H, W, gap, id_limit, pl.words, (const int*)L,
                       (const int*)cmin, (const int*)cmax, bits);
    if (pl.Zi > 0) {
        hipLaunchKernelGGL(mg_rootstate_kernel, dim3(mg_blocks(nI)), dim3(256), 0, s, pl.HW, nI, (const int*)L, (const int*)cmin, cmax);
        hipLaunchKernelGGL(mg_survive_kernel, dim3(mg_blocks(nI)), dim3(256), 0, s, labels, pl.HW, gap, id_limit, pl.words, nI, (const int*)L,
                           cmax, (const unsigned*)bits);
        hipLaunchKernelGGL(mg_count_kernel, dim3((unsigned)(pl.Zi * pl.nb)), dim3(256), 0, s, pl.HW, pl.nb, (const int*)L, (const int*)cmax, bcnt);
    }
    hipLaunchKernelGGL(mg_scan_kernel, dim3((unsigned)Z), dim3(256), 0, s, Z, gap, pl.words, pl.nb, (const unsigned*)bits, wpre, nids, bcnt, nkept);
    hipLaunchKernelGGL(mg_offset_kernel, dim3(1), dim3(64), 0, s, Z, gap, (const int*)nids, (const int*)nkept, off, result);
    if (pl.Zi > 0)
        hipLaunchKernelGGL(mg_rank_kernel, dim3((unsigned)(pl.Zi * pl.nb)), dim3(256), 0, s, pl.HW, pl.nb, (const int*)L, (const int*)cmax,
                           (const int*)bcnt, cmin);
    hipLaunchKernelGGL(mg_paint_kernel, dim3(mg_blocks(nA)), dim3(256), 0, s, labels, Z, H, W, gap, id_limit, pl.words, (const int*)L,
                       (const int*)cmin, (const int*)cmax, (const unsigned*)bits, (const int*)wpre, (const int*)nkept, (const int*)off, out,
                       result);
    return msam_check_launch("msam_close_gaps");
}

extern "C" int msam_label_z_ranges(const int32_t* labels, int32_t Z, int32_t H, int32_t W, int32_t n_ids, int32_t* zr, int32_t* flag,
                                   void* stream) {
    if (!labels || !zr || !flag) { msam_set_error("msam_label_z_ranges: null pointer"); return 1; }
    const long HW = (long)H * W;
    if (Z < 1 || H < 1 || W < 1 || HW >= (1L << 31) || (long)Z * HW >= (1L << 38)) { msam_set_error("msam_label_z_ranges" MG_SHAPE_MSG); return 1; }
    if (n_ids < 1 || n_ids > (1 << 30)) { msam_set_error("msam_label_z_ranges: 1 <= n_ids <= 2^30"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) { msam_set_error("msam_label_z_ranges: memset failed"); return 2; }
    hipLaunchKernelGGL(mg_zr_init_kernel, dim3(mg_blocks(n_ids)), dim3(256), 0, s, n_ids, Z, zr);
    hipLaunchKernelGGL(mg_zr_kernel, dim3(mg_blocks((long)Z * HW)), dim3(256), 0, s, labels, Z, W, HW, n_ids, zr, flag);
    return msam_check_launch("msam_label_z_ranges");
}

extern "C" int msam_apply_label_lut(const int32_t* labels, int64_t n, const int32_t* lut, int32_t n_lut, int32_t* out, int32_t* flag,
                                    void* stream) {
    if (!labels || !lut || !out || !flag) { msam_set_error("msam_apply_label_lut: null pointer"); return 1; }
    if (n < 1 || n >= (1L << 38) || n_lut < 1) { msam_set_error("msam_apply_label_lut: 1 <= n < 2^38 and n_lut >= 1"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) { msam_set_error("msam_apply_label_lut: memset failed"); return 2; }
    hipLaunchKernelGGL(mg_lut_kernel, dim3(mg_blocks(n)), dim3(256), 0, s, labels, (long)n, lut, n_lut, out, flag);
    return msam_check_launch("msam_apply_label_lut");
}
