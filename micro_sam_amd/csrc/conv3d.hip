// The convolutions of the two 3-d wrappers as implicit GEMMs on bf16 rows [M, Ci], and the InstanceNorm of the volumetric decoder:
//   * msam_conv3d_k3_bf16: Conv3d(Ci, Co, 3, padding=1) of models/simple_sam_3d_wrapper.py (BasicBlock, SegmentationHead) on
//     CHANNELS-LAST voxel rows - a tensor [B, D, H, W, C] is the row matrix [B D H W, C], row ((b D + z) H + y) W + x;
//   * msam_depth_conv3_bf16: Conv3d(C, C, (3, 1, 1), padding="same") of models/sam_3d_wrapper.py (NDBlockWrapper) on TOKEN-MAJOR rows
//     [B D T, C], row (b D + z) T + t.
//
// 1. The forward tile body, conv_taps_kernel<Geom, WM, WN, FM, FN>: K = TAPS Ci (rounded up to the k-tile of 64),
//        out[m, co] = bias[co] + sum_{tap, ci} W[co, tap Ci + ci] x[m + tap_rows(tap), ci],   a term dropped when the tap leaves the volume.
//    A (the im2col matrix [M, TAPS Ci]) is never written.  128 x BN x 64 tiles, 256 threads, v_mfma_f32_16x16x32_bf16, two LDS buffers with
//    XOR-swizzled 128-B rows (common.h swz), global -> VGPR two k-tiles ahead -> ds_write, C staged through LDS for 16-byte stores, XCD
//    remap.
//    * A geometry (CubeGeom, DepthGeom) supplies the number of taps, a row's mask of the taps inside its volume, the tap of a k and the
//      rows from a voxel to its neighbour of a tap; nothing else in the body depends on it.
//        cube:  TAPS = 27, tap = (kz 3 + ky) 3 + kx, tap_rows = ((kz - 1) H + (ky - 1)) W + (kx - 1)
//        depth: TAPS = 3,  tap = kz,                 tap_rows = (kz - 1) T        (T need not divide the tile: the mask is per row)
//    * The A-side address: every staged row carries its mask, and the tap is chosen PER 16-BYTE CHUNK (k = tap Ci + ci with Ci % 8 == 0,
//      so a chunk never straddles two taps, but with Ci < 64 one 64-wide k-tile does).  A chunk whose tap lies outside the volume, whose
//      row is past M or whose k lies in the padding of K is loaded from a LEGAL address - channel 0 of its own row, the row clamped to
//      M - 1 - and zeroed in registers; no address outside x is formed, also not for the first slice of the first volume and the last
//      slice of the last one.
//    * The N tile: BN = 128 (2 x 2 waves of 4 x 4 fragments), 64, 32, 16 (4 x 1 waves of 2 x 4 / 2 x 2 / 2 x 1) from one template.  The
//      cube launcher takes the largest that divides Co; the depth launcher always 128.
//    The input gradient is the same call on W' (include/msam_hip.h).
// 2. msam_conv3d_k3_wgrad_bf16: dW[tap Ci + ci, co] = sum_m x[m + shift(tap), ci] dy[m, co], the same implicit A contracted over the
//    voxels.  Both operands are channels-last, i.e. strided along the contraction: a workgroup stages 64 voxels of a 64-wide k-tile of A
//    (same address rule) and of dy TRANSPOSED into LDS (2-byte writes) and feeds mfma16 from 16-byte reads along the voxels.  The voxels
//    are split over workgroups; the partial tiles go to a caller-provided workspace and are added in split order by a second kernel.
// 3. InstanceNorm3d (no affine, biased variance) on fp32 rows: per-workgroup fp64 partial sums in a caller-provided workspace, added in
//    index order; the fused apply (two normalised operands, LeakyReLU) and the closed-form backward (one statistics pass + one
//    elementwise pass).  msam_column_sums_f32 (the bias gradient) is the statistics pass with one accumulator.
// No atomics anywhere; every output element is one fixed-order sum: two calls agree bit for bit.
#include "common.h"
#include <cmath>
#include <cstdio>
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int C3_BM = 128, C3_BK = 64;
constexpr int C3_ACH = C3_BM * 8;           // 16-B chunks of an A tile
constexpr int C3_MAX_CI = 4096;             // c3_div below is exact for k < 27 * 4096 + 64

MSAM_DEVINL uint4 c3_keep(const uint4& v, bool keep) {
    uint4 r;
    r.x = keep ? v.x : 0u; r.y = keep ? v.y : 0u; r.z = keep ? v.z : 0u; r.w = keep ? v.w : 0u;
    return r;
}

// k / Ci by multiplication: magic = 2^32 / Ci + 1 is exact while k (magic Ci - 2^32) < 2^32, i.e. for every k <= 27 Ci + 63, Ci <= 4096
MSAM_DEVINL int c3_div(int k, unsigned magic) { return (int)(((unsigned long long)(unsigned)k * magic) >> 32); }

// bit tap = (kz 3 + ky) 3 + kx set: voxel row m reads tap inside its volume
MSAM_DEVINL int c3_row_mask(int m, int D, int H, int W) {
    const int x = m % W, t = m / W, y = t % H, z = (t / H) % D;
    const int mx = (x > 0 ? 1 : 0) | 2 | (x < W - 1 ? 4 : 0);
    const int my = (y > 0 ? 1 : 0) | 2 | (y < H - 1 ? 4 : 0);
    const int mz = (z > 0 ? 1 : 0) | 2 | (z < D - 1 ? 4 : 0);
    int mask = 0;
#pragma unroll
    for (int kz = 0; kz < 3; ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
            if (((mz >> kz) & 1) && ((my >> ky) & 1)) mask |= mx << ((kz * 3 + ky) * 3);
    return mask;
}

// rows from a voxel to its neighbour of tap (tap < 27)
MSAM_DEVINL int c3_tap_rows(int tap, int H, int W) {
    const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
    return ((kz - 1) * H + (ky - 1)) * W + (kx - 1);
}

// The geometries of conv_taps_kernel.  row_mask(m): bit tap set = voxel row m reads tap inside its volume; tap_of(k): the tap of column k
// of A (>= TAPS in the padding of K); tap_rows(tap): rows from a voxel to its neighbour of tap (tap < TAPS)
struct CubeGeom {
    static constexpr int TAPS = 27;
    int D, H, W;
    unsigned magic;                                        // of Ci <= C3_MAX_CI (c3_div)
    __device__ __forceinline__ int row_mask(int m) const { return c3_row_mask(m, D, H, W); }
    __device__ __forceinline__ int tap_of(int k) const { return c3_div(k, magic); }
    __device__ __forceinline__ int tap_rows(int tap) const { return c3_tap_rows(tap, H, W); }
};

struct DepthGeom {                                         // K = 3 Ci exactly: no padding, and two compares are exact for every Ci
    static constexpr int TAPS = 3;
    int D, T, Ci;
    __device__ __forceinline__ int row_mask(int m) const {
        const int z = (m / T) % D;
        return (z > 0 ? 1 : 0) | 2 | (z < D - 1 ? 4 : 0);
    }
    // Ci % 64 == 0: a k-tile never mixes taps, so the tap is that of the k-tile's first column - one scalar value per k-tile
    __device__ __forceinline__ int tap_of(int k) const {
        const int k0 = k & ~(C3_BK - 1);
        return (k0 >= Ci ? 1 : 0) + (k0 >= 2 * Ci ? 1 : 0);
    }
    __device__ __forceinline__ int tap_rows(int tap) const { return (tap - 1) * T; }
};

template <class Geom, int WM, int WN, int FM, int FN>
__global__ __launch_bounds__(256, 2) void conv_taps_kernel(const u16* __restrict__ X, long ldx, const u16* __restrict__ Wt,
                                                           const float* __restrict__ bias, float* __restrict__ out, long ldc, int M,
                                                           int Ci, int Co, int Kp, Geom geom) {
    constexpr int BN = WN * FN * 16;
    constexpr int BCH = BN * 8;                            // 16-B chunks of a W tile
    constexpr int WP = (BCH + 255) / 256;                  // ... per thread
    static_assert(WM * WN == 4 && WM * FM * 16 == C3_BM, "4 waves cover the 128 rows");
    __shared__ __attribute__((aligned(16))) uint4 lds[2 * C3_ACH + 2 * BCH];   // A buffers 0 / 1, then W buffers 0 / 1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = Co / BN, tiles_m = (M + C3_BM - 1) / C3_BM;
    // XCD-aware remap (bijective): consecutive tiles (sharing the A panel) run on one XCD / one L2
    int nwg = tiles_m * tiles_n, bid = (int)blockIdx.x;
    {
        int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
    const int m0 = tile_m * C3_BM, n0 = tile_n * BN;
    const int wm = wave / WN, wn = wave % WN;

    // staging map: thread t covers LDS chunk position (row = pass*32 + t/8, c' = t%8), which holds global chunk c' ^ swz(row).
    // aoff: byte offset of channel 0 of the row itself (clamped to M - 1); ok: the row's tap mask (0 for a row past M);
    // ak: the chunk's k inside a k-tile
    const int srow = tid >> 3, scp = tid & 7;
    int aoff[4], ok[4], ak[4], woff[WP];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int row = p * 32 + srow;
        const int m = m0 + row;
        const int ar = m > M - 1 ? M - 1 : m;
        ok[p] = m < M ? geom.row_mask(ar) : 0;
        aoff[p] = (int)((long)ar * ldx * 2);
        ak[p] = (scp ^ swz(row)) * 8;
    }
    const bool wlive = BCH >= 256 || tid < BCH;            // BN = 16: the W tile has 128 chunks
#pragma unroll
    for (int p = 0; p < WP; ++p) {
        const int row = wlive ? p * 32 + srow : 0;
        woff[p] = (int)(((long)(n0 + row) * Kp + (scp ^ swz(row)) * 8) * 2);
    }
    const int ldx2 = (int)(ldx * 2);

    f32x4_t acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nk = Kp / C3_BK;
    const int fr = lane & 15, fg = lane >> 4;
    auto compute = [&](int buf) {
        const uint4* la = lds + buf * C3_ACH;
        const uint4* lb = lds + 2 * C3_ACH + buf * BCH;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 a[FM], b[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int row = (wm * FM + i) * 16 + fr;
                a[i] = la[row * 8 + ((ks * 4 + fg) ^ swz(row))];
            }
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                const int col = (wn * FN + j) * 16 + fr;
                b[j] = lb[col * 8 + ((ks * 4 + fg) ^ swz(col))];
            }
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        }
    };

    // the descriptors end with the last element the kernel may read: (M - 1) ldx + Ci of x, Co rows of W (the launcher keeps both
    // below 2^31 bytes, so the per-lane offsets are plain non-negative ints)
    const rsrc_t rx = make_rsrc(X, (uint32_t)((((long)M - 1) * ldx + Ci) * 2));
    const rsrc_t rw = make_rsrc(Wt, (uint32_t)((long)Co * Kp * 2));
    // k-tile kt: chunk p of this thread holds k = kt 64 + ak[p] .. + 7 = channels ci .. ci + 7 of tap k / Ci.  A chunk that counts reads
    // row m + tap_rows(tap) (inside x: the mask says so); any other chunk channel 0 of its own row.  keep: bit p = chunk p counts
    auto load = [&](uint4 (&a)[4], uint4 (&w)[WP], int& keep, int kt) {
        keep = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int k = kt * C3_BK + ak[p];
            const int tap = geom.tap_of(k);
            const bool on = tap < Geom::TAPS && ((ok[p] >> (tap & 31)) & 1);
            // worked out for every chunk and masked, not selected: a thread's four chunks share k, so they share this value, and the
            // compiler keeps it out of an exec-mask region per load (unsigned: the value of a chunk that does not count may wrap)
            const unsigned off = (unsigned)geom.tap_rows(tap) * (unsigned)ldx2 + (unsigned)(k - tap * Ci) * 2u;
            const int rel = (int)(off & (on ? ~0u : 0u));
            a[p] = buf_load16(rx, aoff[p] + rel, 0);
            keep |= (on ? 1 : 0) << p;
        }
#pragma unroll
        for (int p = 0; p < WP; ++p) w[p] = buf_load16(rw, woff[p], kt * C3_BK * 2);
    };
    auto commit = [&](const uint4 (&a)[4], const uint4 (&w)[WP], int keep, int buf) {
        uint4* la = lds + buf * C3_ACH;
        uint4* lb = lds + 2 * C3_ACH + buf * BCH;
#pragma unroll
        for (int p = 0; p < 4; ++p) la[(p * 32 + srow) * 8 + scp] = c3_keep(a[p], (keep >> p) & 1);
        if (wlive) {
#pragma unroll
            for (int p = 0; p < WP; ++p) lb[(p * 32 + srow) * 8 + scp] = w[p];
        }
    };
    uint4 ra[4], rwv[WP], sa[4], swv[WP];
    int rkeep, skeep = 0;
    // register staging TWO k-tiles ahead (two register sets, roles swapped by the 2x unrolled loop), as gemm.hip; nk >= 3 always
    load(ra, rwv, rkeep, 0);
    commit(ra, rwv, rkeep, 0);
    load(ra, rwv, rkeep, 1);
    __syncthreads();
    int kt = 0;
    while (true) {
        load(sa, swv, skeep, min(kt + 2, nk - 1));
        compute(kt & 1);
        if (kt + 1 < nk) commit(ra, rwv, rkeep, (kt & 1) ^ 1);
        __syncthreads();
        if (++kt >= nk) break;
        load(ra, rwv, rkeep, min(kt + 2, nk - 1));
        compute(kt & 1);
        if (kt + 1 < nk) commit(sa, swv, skeep, (kt & 1) ^ 1);
        __syncthreads();
        if (++kt >= nk) break;
    }
    wait_vmem_all();                                       // the clamped tail prefetches must not outlive the LDS reuse below

    // ---- epilogue: the fp32 C tile through LDS (the operand buffers), then 4 consecutive columns of one row per thread and pass
    float* ldsC = (float*)&lds[0];                         // [128][BN] fp32 <= the operand buffers
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ldsC[((wm * FM + i) * 16 + fg * 4 + r) * BN + (wn * FN + j) * 16 + fr] = acc[i][j][r];
    __syncthreads();

    constexpr int TPR = BN / 4;                            // threads per row
    constexpr int RPP = 256 / TPR;                         // rows per pass
    const int c4 = (tid % TPR) * 4;
    const int col = n0 + c4;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) b4 = *(const float4*)(bias + col);
    const int lr0 = tid / TPR;
#pragma unroll
    for (int pass = 0; pass < C3_BM / RPP; ++pass) {
        const int lr = pass * RPP + lr0;
        const int row = m0 + lr;
        if (row >= M) break;                               // rows only grow with pass; no barrier inside the loop
        const float4 c = *(const float4*)(ldsC + lr * BN + c4);
        *(float4*)(out + (long)row * ldc + col) = make_float4(c.x + b4.x, c.y + b4.y, c.z + b4.z, c.w + b4.w);
    }
}

// ---- weight gradient.  Workgroup (kt, ct; split): the 64 x (16 NF) tile k = kt 64 .., co = ct 16 NF .. of dW^T over the voxel tiles
// [split tps, (split + 1) tps).  Thread t stages chunk (row = p 32 + t / 8, k = kt 64 + (t % 8) 8): its tap is the same for every voxel
constexpr int WG_LD = 72;                                  // LDS row: 64 voxels + 8 (16-byte aligned rows, staggered banks)

template <int NF>
__global__ __launch_bounds__(256) void conv3d_k3_wgrad_kernel(const u16* __restrict__ X, long ldx, const u16* __restrict__ DY, long ldy,
                                                              float* __restrict__ part, int M, int D, int H, int W, int Ci, int Co,
                                                              unsigned magic, int ktiles, int tps) {
    constexpr int BC = NF * 16;
    constexpr int YCH = 64 * BC / 8;                       // 16-B chunks of a dy tile
    constexpr int YP = (YCH + 255) / 256;
    __shared__ __attribute__((aligned(16))) u16 xt[64 * WG_LD];
    __shared__ __attribute__((aligned(16))) u16 yt[BC * WG_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int K = 27 * Ci;
    const int kt = (int)blockIdx.x % ktiles, ct = (int)blockIdx.x / ktiles;
    const int k0 = kt * 64, n0 = ct * BC;
    const int mtiles = (M + 63) / 64;
    const int mt0 = (int)blockIdx.y * tps, mt1 = min(mt0 + tps, mtiles);

    const int gc = tid & 7, srow = tid >> 3;
    const int kc = k0 + gc * 8;
    const int tap = c3_div(kc, magic);
    const bool tap_ok = tap < 27;
    const int dz = tap_ok ? tap / 9 - 1 : 0, dy_ = tap_ok ? (tap / 3) % 3 - 1 : 0, dx = tap_ok ? tap % 3 - 1 : 0;
    const int rel = tap_ok ? (int)((long)((dz * H + dy_) * W + dx) * ldx * 2) + (kc - tap * Ci) * 2 : 0;
    const rsrc_t rx = make_rsrc(X, (uint32_t)((((long)M - 1) * ldx + Ci) * 2));
    const rsrc_t ry = make_rsrc(DY, (uint32_t)((((long)M - 1) * ldy + Co) * 2));

    f32x4_t acc[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    for (int mt = mt0; mt < mt1; ++mt) {
        const int m0 = mt * 64;
        uint4 xv[2], yv[YP];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int m = m0 + p * 32 + srow;
            const int ar = m > M - 1 ? M - 1 : m;
            const int x_ = ar % W, t_ = ar / W, y_ = t_ % H, z_ = (t_ / H) % D;
            const bool on = m < M && tap_ok && (unsigned)(z_ + dz) < (unsigned)D && (unsigned)(y_ + dy_) < (unsigned)H &&
                            (unsigned)(x_ + dx) < (unsigned)W;
            xv[p] = c3_keep(buf_load16(rx, (int)((long)ar * ldx * 2) + (on ? rel : 0), 0), on);
        }
#pragma unroll
        for (int p = 0; p < YP; ++p) {
            const int q = p * 256 + tid;                   // chunk (row = q / (BC / 8), columns (q % (BC / 8)) 8 ..) of the dy tile
            const int row = (q / (BC / 8)) & 63, co = n0 + (q % (BC / 8)) * 8;
            const int m = m0 + row;
            const int ar = m > M - 1 ? M - 1 : m;
            const bool on = m < M && co < Co && q < YCH;
            yv[p] = c3_keep(buf_load16(ry, (int)((long)ar * ldy * 2) + (on ? co * 2 : 0), 0), on);
        }
        // transposed into LDS: [k or co][voxel]
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const uint32_t wds[4] = {xv[p].x, xv[p].y, xv[p].z, xv[p].w};
#pragma unroll
            for (int i = 0; i < 8; ++i) xt[(gc * 8 + i) * WG_LD + p * 32 + srow] = (u16)(wds[i >> 1] >> (16 * (i & 1)));
        }
#pragma unroll
        for (int p = 0; p < YP; ++p) {
            const int q = p * 256 + tid;
            if (q < YCH) {
                const int row = q / (BC / 8), c8 = (q % (BC / 8)) * 8;
                const uint32_t wds[4] = {yv[p].x, yv[p].y, yv[p].z, yv[p].w};
#pragma unroll
                for (int i = 0; i < 8; ++i) yt[(c8 + i) * WG_LD + row] = (u16)(wds[i >> 1] >> (16 * (i & 1)));
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const uint4 a = *(const uint4*)(xt + (wave * 16 + fr) * WG_LD + (ks * 4 + fg) * 8);
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const uint4 b = *(const uint4*)(yt + (j * 16 + fr) * WG_LD + (ks * 4 + fg) * 8);
                acc[j] = mfma16(a, b, acc[j]);
            }
        }
        __syncthreads();
    }
    float* dst = part + (long)blockIdx.y * K * Co;
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + wave * 16 + fg * 4 + r, co = n0 + j * 16 + fr;
            if (k < K && co < Co) dst[(long)k * Co + co] = acc[j][r];
        }
}

__global__ __launch_bounds__(256) void conv3d_k3_wgrad_sum_kernel(const float* __restrict__ part, float* __restrict__ dw, int n, int splits) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int sp = 1; sp < splits; ++sp) s += part[(long)sp * n + i];      // split order: the same bits on every run
    dw[i] = s;
}

struct WgradPlan { int nf, cotiles, ktiles, splits, tps; };

WgradPlan wgrad_plan(int64_t M, int Ci, int Co) {
    WgradPlan p;
    p.nf = Co <= 16 ? 1 : Co <= 32 ? 2 : Co <= 64 ? 4 : 8;
    p.cotiles = (Co + p.nf * 16 - 1) / (p.nf * 16);
    p.ktiles = (27 * Ci + 63) / 64;
    const int64_t mtiles = (M + 63) / 64;
    int64_t want = 1024 / ((int64_t)p.ktiles * p.cotiles);
    if (want < 1) want = 1;
    if (want > mtiles) want = mtiles;
    p.tps = (int)((mtiles + want - 1) / want);
    p.splits = (int)((mtiles + p.tps - 1) / p.tps);
    return p;
}

// ---- InstanceNorm.  Rows [B V, C] fp32, C a power of two in 4 .. 1024: thread t owns the four columns (t % (C / 4)) 4 .. and every
// (256 / (C / 4))-th row of its workgroup's chunk of a volume.
struct InArgs {
    const float* a; long lda; const double* sa;            // sa / sr: (mean, variance) per (b, c)
    const float* r; long ldr; const double* sr;
    const float* dy; long ldy;
    double* part;
    int V, C, rows, nchunks;
    float eps, slope;
    int has_act;
};

MSAM_DEVINL float in_rstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }
MSAM_DEVINL float in_get(const float4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

struct InCols {                                            // the statistics of a thread's four columns
    double mean[4]; float rstd[4];
};
MSAM_DEVINL InCols in_cols(const double* s, int b, int C, int c0, float eps) {
    InCols o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o.mean[q] = s[((long)b * C + c0 + q) * 2];
        o.rstd[q] = in_rstd(s[((long)b * C + c0 + q) * 2 + 1], eps);
    }
    return o;
}

// MODE 0: sum x, sum x^2.  MODE 1: sum x.  MODE 2: sum g, sum g ahat, sum g rhat (g = dy act'(ahat + rhat))
template <int MODE>
__global__ __launch_bounds__(256) void in_partial_kernel(InArgs p) {
    constexpr int NACC = MODE == 0 ? 2 : MODE == 1 ? 1 : 3;
    __shared__ double red[256 * 4];
    const int tid = threadIdx.x;
    const int tc = p.C / 4, rp = 256 / tc;
    const int c0 = (tid % tc) * 4, trow = tid / tc;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int v0 = chunk * p.rows, v1 = min(v0 + p.rows, p.V);
    double s[NACC][4];
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[i][q] = 0.0;
    InCols ca, cr;
    if (MODE == 2) {
        ca = in_cols(p.sa, b, p.C, c0, p.eps);
        if (p.r) cr = in_cols(p.sr, b, p.C, c0, p.eps);
    }
    for (int v = v0 + trow; v < v1; v += rp) {
        const long row = (long)b * p.V + v;
        const float4 a4 = *(const float4*)(p.a + row * p.lda + c0);
        if (MODE == 2) {
            const float4 g4 = *(const float4*)(p.dy + row * p.ldy + c0);
            float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.r) r4 = *(const float4*)(p.r + row * p.ldr + c0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float ah = (float)((double)in_get(a4, q) - ca.mean[q]) * ca.rstd[q];
                const float rh = p.r ? (float)((double)in_get(r4, q) - cr.mean[q]) * cr.rstd[q] : 0.f;
                const float pre = ah + rh;
                const float g = in_get(g4, q) * ((p.has_act && !(pre > 0.f)) ? p.slope : 1.f);
                s[0][q] += (double)g;
                s[NACC > 1 ? 1 : 0][q] += (double)g * (double)ah;
                if (NACC > 2) s[NACC > 2 ? 2 : 0][q] += (double)g * (double)rh;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double x = (double)in_get(a4, q);
                s[0][q] += x;
                if (MODE == 0) s[NACC > 1 ? 1 : 0][q] += x * x;
            }
        }
    }
    // the rp thread rows of the workgroup, added in row order by the first one
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[tid * 4 + q] = s[i][q];
        __syncthreads();
        if (trow == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double t = red[tid * 4 + q];
                for (int j = 1; j < rp; ++j) t += red[(j * tc + tid) * 4 + q];
                p.part[(((long)b * p.nchunks + chunk) * NACC + i) * p.C + c0 + q] = t;
            }
        }
        __syncthreads();
    }
}

// out[(b C + c) nacc + i] = scale * sum over the chunks in index order; to_var: the second value becomes E[x^2] - E[x]^2 (>= 0)
__global__ __launch_bounds__(256) void in_final_kernel(const double* __restrict__ part, double* __restrict__ out, int BC, int C,
                                                       int nchunks, int nacc, double scale, int to_var) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i % C;
    double vals[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nacc; ++k) {
        double s = 0.0;
        for (int ch = 0; ch < nchunks; ++ch) s += part[(((long)b * nchunks + ch) * nacc + k) * C + c];
        vals[k] = s * scale;
    }
    if (to_var) { const double v = vals[1] - vals[0] * vals[0]; vals[1] = v > 0.0 ? v : 0.0; }
    for (int k = 0; k < nacc; ++k) out[(long)i * nacc + k] = vals[k];
}

// y = act(ahat + rhat) to fp32 and / or bf16 rows
__global__ __launch_bounds__(256) void in_apply_kernel(InArgs p, long quads, float* __restrict__ o32, long ld32, u16* __restrict__ o16,
                                                       long ld16) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const int tc = p.C / 4;
    const long row = i / tc;
    const int c0 = (int)(i % tc) * 4;
    const int b = (int)(row / p.V);
    const InCols ca = in_cols(p.sa, b, p.C, c0, p.eps);
    const float4 a4 = *(const float4*)(p.a + row * p.lda + c0);
    float y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) y[q] = (float)((double)in_get(a4, q) - ca.mean[q]) * ca.rstd[q];
    if (p.r) {
        const InCols cr = in_cols(p.sr, b, p.C, c0, p.eps);
        const float4 r4 = *(const float4*)(p.r + row * p.ldr + c0);
#pragma unroll
        for (int q = 0; q < 4; ++q) y[q] += (float)((double)in_get(r4, q) - cr.mean[q]) * cr.rstd[q];
    }
    if (p.has_act) {
#pragma unroll
        for (int q = 0; q < 4; ++q) y[q] = y[q] > 0.f ? y[q] : y[q] * p.slope;
    }
    if (o32) *(float4*)(o32 + row * ld32 + c0) = make_float4(y[0], y[1], y[2], y[3]);
    if (o16) *(uint2*)(o16 + row * ld16 + c0) = make_uint2(pack2bf(y[0], y[1]), pack2bf(y[2], y[3]));
}

// da = rstd_a (g - mean(g) - ahat mean(g ahat)), dr likewise; sums: (mean g, mean g ahat, mean g rhat) per (b, c)
__global__ __launch_bounds__(256) void in_backward_kernel(InArgs p, long quads, const double* __restrict__ sums, float* __restrict__ da,
                                                          long ldda, float* __restrict__ dr, long lddr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= quads) return;
    const int tc = p.C / 4;
    const long row = i / tc;
    const int c0 = (int)(i % tc) * 4;
    const int b = (int)(row / p.V);
    const InCols ca = in_cols(p.sa, b, p.C, c0, p.eps);
    InCols cr;
    if (p.r) cr = in_cols(p.sr, b, p.C, c0, p.eps);
    const float4 a4 = *(const float4*)(p.a + row * p.lda + c0);
    const float4 g4 = *(const float4*)(p.dy + row * p.ldy + c0);
    float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.r) r4 = *(const float4*)(p.r + row * p.ldr + c0);
    float oa[4], orr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double* sm = sums + ((long)b * p.C + c0 + q) * 3;
        const float ah = (float)((double)in_get(a4, q) - ca.mean[q]) * ca.rstd[q];
        const float rh = p.r ? (float)((double)in_get(r4, q) - cr.mean[q]) * cr.rstd[q] : 0.f;
        const float pre = ah + rh;
        const float g = in_get(g4, q) * ((p.has_act && !(pre > 0.f)) ? p.slope : 1.f);
        const float m1 = (float)sm[0];
        oa[q] = ca.rstd[q] * (g - m1 - ah * (float)sm[1]);
        orr[q] = p.r ? cr.rstd[q] * (g - m1 - rh * (float)sm[2]) : 0.f;
    }
    *(float4*)(da + row * ldda + c0) = make_float4(oa[0], oa[1], oa[2], oa[3]);
    if (p.r && dr) *(float4*)(dr + row * lddr + c0) = make_float4(orr[0], orr[1], orr[2], orr[3]);
}

struct InPlan { int rows, nchunks; };
InPlan in_plan(int64_t V, int C) {
    const int rp = 256 / (C / 4);
    int64_t rows = (V + 1023) / 1024;                      // at most 1024 chunks per volume
    if (rows < 64) rows = 64;
    rows = (rows + rp - 1) / rp * rp;
    InPlan p;
    p.rows = (int)rows;
    p.nchunks = (int)((V + rows - 1) / rows);
    return p;
}

bool in_pow2(int c) { return c >= 4 && c <= 1024 && (c & (c - 1)) == 0; }

// the checks every InstanceNorm entry shares; `ld` fp32 row strides (0: operand absent)
int in_check(const char* who, int B, int64_t V, int C, const void* const* ptrs, const int64_t* lds, int n) {
    char msg[320];
    if (B < 1 || V < 1 || !in_pow2(C) || (int64_t)B * V >= (1LL << 31)) {
        snprintf(msg, sizeof msg, "%s: needs B, V >= 1, B V < 2^31 and C a power of two in 4 .. 1024, got B = %d, V = %lld, C = %d", who, B,
                 (long long)V, C);
        msam_set_error(msg);
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        if (!ptrs[i]) continue;
        if ((uintptr_t)ptrs[i] % 16 != 0 || lds[i] < C || lds[i] % 4 != 0) {
            snprintf(msg, sizeof msg, "%s: operand %d must be 16-byte aligned with a row stride >= C in fours, got a stride of %lld", who, i,
                     (long long)lds[i]);
            msam_set_error(msg);
            return 1;
        }
    }
    return 0;
}

int64_t in_ws_bytes(int B, int64_t V, int C) { return (int64_t)B * in_plan(V, C).nchunks * 3 * C * (int64_t)sizeof(double); }

}  // namespace

// The checks msam_conv3d_k3_bf16 and msam_depth_conv3_bf16 share, in the order null pointers (conv_null_check; the entry's own shape rules
// come next), strides, 2^31 limits, alignment.  `who`: the entry's name; `rows`: how it spells M; Kp: the row length of W; BN: its N tile
static int conv_null_check(const char* who, const void* x, const void* w, const void* out) {
    char msg[128];
    if (x && w && out) return 0;
    snprintf(msg, sizeof msg, "%s: null pointer", who);
    msam_set_error(msg);
    return 1;
}

static int conv_operand_check(const char* who, const char* rows, const void* x, int64_t ldx, const void* w, const float* bias,
                              const float* out, int64_t ldc, int64_t M, int32_t Ci, int32_t Co, int64_t Kp, int BN) {
    char msg[384];
    if (ldx < Ci || ldc < Co || ldx % 8 != 0 || ldc % 4 != 0) {
        snprintf(msg, sizeof msg, "%s: needs ldx >= Ci in eights and ldc >= Co in fours, got ldx = %lld, ldc = %lld", who, (long long)ldx,
                 (long long)ldc);
        msam_set_error(msg);
        return 1;
    }
    if (M >= (1LL << 31) || M * ldx * 2 >= (1LL << 31) || (int64_t)Co * Kp * 2 >= (1LL << 31) ||
        ((M + C3_BM - 1) / C3_BM) * (Co / BN) >= (1LL << 31)) {
        snprintf(msg, sizeof msg, "%s: x (%s rows of ldx) and W must stay below 2^31 bytes each, got %lld rows of %lld", who, rows,
                 (long long)M, (long long)ldx);
        msam_set_error(msg);
        return 1;
    }
    if ((uintptr_t)x % 16 != 0 || (uintptr_t)w % 16 != 0 || (uintptr_t)out % 16 != 0 || (bias && (uintptr_t)bias % 16 != 0)) {
        snprintf(msg, sizeof msg, "%s: x, w, bias and out must be 16-byte aligned", who);
        msam_set_error(msg);
        return 1;
    }
    return 0;
}

#define CONV_LAUNCH(GEOM_, WM_, WN_, FM_, FN_, geom_)                                                                                    \
    hipLaunchKernelGGL((conv_taps_kernel<GEOM_, WM_, WN_, FM_, FN_>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const u16*)x,     \
                       (long)ldx, (const u16*)w, bias, out, (long)ldc, (int)M, (int)Ci, (int)Co, (int)Kp, geom_)

extern "C" int msam_conv3d_k3_bf16(const void* x, int64_t ldx, const void* w, const float* bias, float* out, int64_t ldc, int32_t B,
                                   int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co, void* stream) {
    char msg[384];
    if (conv_null_check("msam_conv3d_k3_bf16", x, w, out)) return 1;
    if (B < 1 || D < 1 || H < 1 || W < 1 || Ci < 8 || Ci % 8 != 0 || Ci > C3_MAX_CI || Co < 16 || Co % 16 != 0) {
        snprintf(msg, sizeof msg, "msam_conv3d_k3_bf16: needs B, D, H, W >= 1, Ci a multiple of 8 in 8 .. %d and Co a positive multiple of 16, "
                                  "got B = %d, D = %d, H = %d, W = %d, Ci = %d, Co = %d", C3_MAX_CI, B, D, H, W, Ci, Co);
        msam_set_error(msg);
        return 1;
    }
    const int64_t M = (int64_t)B * D * H * W;
    const int64_t Kp = ((int64_t)27 * Ci + 63) / 64 * 64;
    const int BN = Co % 128 == 0 ? 128 : Co % 64 == 0 ? 64 : Co % 32 == 0 ? 32 : 16;
    if (conv_operand_check("msam_conv3d_k3_bf16", "B D H W", x, ldx, w, bias, out, ldc, M, Ci, Co, Kp, BN)) return 1;
    const unsigned tiles = (unsigned)(((M + C3_BM - 1) / C3_BM) * (Co / BN));
    const CubeGeom geom = {(int)D, (int)H, (int)W, (unsigned)((1ULL << 32) / (unsigned)Ci + 1)};
    if (BN == 128) CONV_LAUNCH(CubeGeom, 2, 2, 4, 4, geom);
    else if (BN == 64) CONV_LAUNCH(CubeGeom, 4, 1, 2, 4, geom);
    else if (BN == 32) CONV_LAUNCH(CubeGeom, 4, 1, 2, 2, geom);
    else CONV_LAUNCH(CubeGeom, 4, 1, 2, 1, geom);
    return msam_check_launch("msam_conv3d_k3_bf16");
}

extern "C" int msam_depth_conv3_bf16(const void* x, int64_t ldx, const void* w, const float* bias, float* out, int64_t ldc, int32_t B,
                                     int32_t D, int32_t T, int32_t Ci, int32_t Co, void* stream) {
    char msg[384];
    if (conv_null_check("msam_depth_conv3_bf16", x, w, out)) return 1;
    if (B < 1 || D < 1 || T < 1 || Ci < 64 || Co < 128 || Ci % 64 != 0 || Co % 128 != 0) {
        snprintf(msg, sizeof msg, "msam_depth_conv3_bf16: needs B, D, T >= 1, Ci a positive multiple of 64 and Co a positive multiple of "
                                  "128, got B = %d, D = %d, T = %d, Ci = %d, Co = %d", B, D, T, Ci, Co);
        msam_set_error(msg);
        return 1;
    }
    const int64_t M = (int64_t)B * D * T;
    const int64_t Kp = (int64_t)3 * Ci;                    // a multiple of the k-tile: no padding
    if (conv_operand_check("msam_depth_conv3_bf16", "B D T", x, ldx, w, bias, out, ldc, M, Ci, Co, Kp, 128)) return 1;
    const unsigned tiles = (unsigned)(((M + C3_BM - 1) / C3_BM) * (Co / 128));
    const DepthGeom geom = {(int)D, (int)T, (int)Ci};
    CONV_LAUNCH(DepthGeom, 2, 2, 4, 4, geom);
    return msam_check_launch("msam_depth_conv3_bf16");
}
#undef CONV_LAUNCH

static int wgrad_check(const char* who, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co) {
    char msg[320];
    if (B < 1 || D < 1 || H < 1 || W < 1 || Ci < 8 || Ci % 8 != 0 || Ci > C3_MAX_CI || Co < 8 || Co % 8 != 0 ||
        (int64_t)B * D * H * W >= (1LL << 31) || (int64_t)27 * Ci * Co >= (1LL << 28)) {
        snprintf(msg, sizeof msg, "%s: needs B, D, H, W >= 1 with fewer than 2^31 voxels, Ci a multiple of 8 in 8 .. %d, Co a positive multiple "
                                  "of 8 and 27 Ci Co < 2^28, got B = %d, D = %d, H = %d, W = %d, Ci = %d, Co = %d", who, C3_MAX_CI, B, D, H, W,
                 Ci, Co);
        msam_set_error(msg);
        return 1;
    }
    return 0;
}

extern "C" int64_t msam_conv3d_k3_wgrad_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co) {
    if (wgrad_check("msam_conv3d_k3_wgrad_workspace_bytes", B, D, H, W, Ci, Co)) return -1;
    const WgradPlan p = wgrad_plan((int64_t)B * D * H * W, Ci, Co);
    return (int64_t)p.splits * 27 * Ci * Co * (int64_t)sizeof(float);
}

extern "C" int msam_conv3d_k3_wgrad_bf16(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, void* workspace,
                                         int64_t workspace_bytes, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                                         void* stream) {
    char msg[320];
    if (!x || !dy || !dw || !workspace) { msam_set_error("msam_conv3d_k3_wgrad_bf16: null pointer"); return 1; }
    if (wgrad_check("msam_conv3d_k3_wgrad_bf16", B, D, H, W, Ci, Co)) return 1;
    const int64_t M = (int64_t)B * D * H * W;
    if (ldx < Ci || ldy < Co || ldx % 8 != 0 || ldy % 8 != 0 || M * ldx * 2 >= (1LL << 31) || M * ldy * 2 >= (1LL << 31)) {
        snprintf(msg, sizeof msg, "msam_conv3d_k3_wgrad_bf16: needs ldx >= Ci and ldy >= Co in eights and x, dy below 2^31 bytes, got %lld "
                                  "rows of %lld and %lld", (long long)M, (long long)ldx, (long long)ldy);
        msam_set_error(msg);
        return 1;
    }
    if ((uintptr_t)x % 16 != 0 || (uintptr_t)dy % 16 != 0 || (uintptr_t)dw % 16 != 0 || (uintptr_t)workspace % 16 != 0) {
        msam_set_error("msam_conv3d_k3_wgrad_bf16: x, dy, dw and the workspace must be 16-byte aligned");
        return 1;
    }
    const WgradPlan p = wgrad_plan(M, Ci, Co);
    const int64_t need = (int64_t)p.splits * 27 * Ci * Co * (int64_t)sizeof(float);
    if (workspace_bytes < need) {
        snprintf(msg, sizeof msg, "msam_conv3d_k3_wgrad_bf16: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                 (long long)need);
        msam_set_error(msg);
        return 1;
    }
    const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)Ci + 1);
    const dim3 grid((unsigned)(p.ktiles * p.cotiles), (unsigned)p.splits);
#define C3_WG(NF_)                                                                                                                     \
    hipLaunchKernelGGL((conv3d_k3_wgrad_kernel<NF_>), grid, dim3(256), 0, (hipStream_t)stream, (const u16*)x, (long)ldx, (const u16*)dy, \
                       (long)ldy, (float*)workspace, (int)M, (int)D, (int)H, (int)W, (int)Ci, (int)Co, magic, p.ktiles, p.tps)
    if (p.nf == 1) C3_WG(1);
    else if (p.nf == 2) C3_WG(2);
    else if (p.nf == 4) C3_WG(4);
    else C3_WG(8);
#undef C3_WG
    const int n = 27 * Ci * Co;
    hipLaunchKernelGGL(conv3d_k3_wgrad_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, dw, n, p.splits);
    return msam_check_launch("msam_conv3d_k3_wgrad_bf16");
}

extern "C" int64_t msam_instance_norm_workspace_bytes(int32_t B, int64_t V, int32_t C) {
    if (in_check("msam_instance_norm_workspace_bytes", B, V, C, nullptr, nullptr, 0)) return -1;
    return in_ws_bytes(B, V, C);
}

static int in_ws_check(const char* who, const void* ws, int64_t have, int64_t need) {
    char msg[256];
    if (!ws || (uintptr_t)ws % 16 != 0 || have < need) {
        snprintf(msg, sizeof msg, "%s: needs a 16-byte aligned workspace of %lld bytes, got %lld", who, (long long)need, (long long)have);
        msam_set_error(msg);
        return 1;
    }
    return 0;
}

extern "C" int msam_column_sums_f32(const float* x, int64_t ldx, int64_t M, int32_t C, double* sums, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    if (!x || !sums) { msam_set_error("msam_column_sums_f32: null pointer"); return 1; }
    const void* ptrs[1] = {x};
    const int64_t lds[1] = {ldx};
    if (in_check("msam_column_sums_f32", 1, M, C, ptrs, lds, 1)) return 1;
    if (in_ws_check("msam_column_sums_f32", workspace, workspace_bytes, in_ws_bytes(1, M, C))) return 1;
    const InPlan pl = in_plan(M, C);
    InArgs p = {};
    p.a = x; p.lda = (long)ldx; p.part = (double*)workspace; p.V = (int)M; p.C = C; p.rows = pl.rows; p.nchunks = pl.nchunks;
    hipLaunchKernelGGL((in_partial_kernel<1>), dim3((unsigned)pl.nchunks, 1u), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(in_final_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, sums,
                       (int)C, (int)C, pl.nchunks, 1, 1.0, 0);
    return msam_check_launch("msam_column_sums_f32");
}

extern "C" int msam_instance_norm_stats(const float* x, int64_t ldx, int32_t B, int64_t V, int32_t C, double* stats, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    if (!x || !stats) { msam_set_error("msam_instance_norm_stats: null pointer"); return 1; }
    const void* ptrs[1] = {x};
    const int64_t lds[1] = {ldx};
    if (in_check("msam_instance_norm_stats", B, V, C, ptrs, lds, 1)) return 1;
    if (V < 2) { msam_set_error("msam_instance_norm_stats: needs more than one value per channel (V >= 2)"); return 1; }
    if (in_ws_check("msam_instance_norm_stats", workspace, workspace_bytes, in_ws_bytes(B, V, C))) return 1;
    const InPlan pl = in_plan(V, C);
    InArgs p = {};
    p.a = x; p.lda = (long)ldx; p.part = (double*)workspace; p.V = (int)V; p.C = C; p.rows = pl.rows; p.nchunks = pl.nchunks;
    hipLaunchKernelGGL((in_partial_kernel<0>), dim3((unsigned)pl.nchunks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(in_final_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                       stats, (int)(B * C), (int)C, pl.nchunks, 2, 1.0 / (double)V, 1);
    return msam_check_launch("msam_instance_norm_stats");
}

extern "C" int msam_instance_norm_apply(const float* a, int64_t lda, const double* stats_a, const float* r, int64_t ldr,
                                        const double* stats_r, int32_t B, int64_t V, int32_t C, float eps, float slope, int32_t has_act,
                                        float* out32, int64_t ld32, void* out16, int64_t ld16, void* stream) {
    if (!a || !stats_a || (r && !stats_r) || (!out32 && !out16)) {
        msam_set_error("msam_instance_norm_apply: null pointer (a, stats_a, stats_r with r, one of out32 / out16)");
        return 1;
    }
    const void* ptrs[4] = {a, r, out32, out16};
    const int64_t lds[4] = {lda, ldr, ld32, ld16};
    if (in_check("msam_instance_norm_apply", B, V, C, ptrs, lds, 4)) return 1;
    if (V < 2 || !(eps >= 0.f)) { msam_set_error("msam_instance_norm_apply: needs V >= 2 and eps >= 0"); return 1; }
    InArgs p = {};
    p.a = a; p.lda = (long)lda; p.sa = stats_a; p.r = r; p.ldr = (long)ldr; p.sr = stats_r; p.V = (int)V; p.C = C; p.eps = eps; p.slope = slope;
    p.has_act = has_act ? 1 : 0;
    const long quads = (long)B * V * (C / 4);
    hipLaunchKernelGGL(in_apply_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, quads, out32, (long)ld32,
                       (u16*)out16, (long)ld16);
    return msam_check_launch("msam_instance_norm_apply");
}

extern "C" int msam_instance_norm_backward(const float* dy, int64_t ldy, const float* a, int64_t lda, const double* stats_a, const float* r,
                                           int64_t ldr, const double* stats_r, int32_t B, int64_t V, int32_t C, float eps, float slope,
                                           int32_t has_act, float* da, int64_t ldda, float* dr, int64_t lddr, double* sums, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    if (!dy || !a || !stats_a || !da || !sums || (r && (!stats_r || !dr))) {
        msam_set_error("msam_instance_norm_backward: null pointer (dy, a, stats_a, da, sums; stats_r and dr with r)");
        return 1;
    }
    const void* ptrs[5] = {dy, a, r, da, r ? dr : nullptr};
    const int64_t lds[5] = {ldy, lda, ldr, ldda, lddr};
    if (in_check("msam_instance_norm_backward", B, V, C, ptrs, lds, 5)) return 1;
    if (V < 2 || !(eps >= 0.f)) { msam_set_error("msam_instance_norm_backward: needs V >= 2 and eps >= 0"); return 1; }
    if (in_ws_check("msam_instance_norm_backward", workspace, workspace_bytes, in_ws_bytes(B, V, C))) return 1;
    const InPlan pl = in_plan(V, C);
    InArgs p = {};
    p.a = a; p.lda = (long)lda; p.sa = stats_a; p.r = r; p.ldr = (long)ldr; p.sr = stats_r; p.dy = dy; p.ldy = (long)ldy;
    p.part = (double*)workspace; p.V = (int)V; p.C = C; p.rows = pl.rows; p.nchunks = pl.nchunks; p.eps = eps; p.slope = slope;
    p.has_act = has_act ? 1 : 0;
    hipLaunchKernelGGL((in_partial_kernel<2>), dim3((unsigned)pl.nchunks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(in_final_kernel, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                       sums, (int)(B * C), (int)C, pl.nchunks, 3, 1.0 / (double)V, 0);
    const long quads = (long)B * V * (C / 4);
    hipLaunchKernelGGL(in_backward_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, quads,
                       (const double*)sums, da, (long)ldda, dr, (long)lddr);
    return msam_check_launch("msam_instance_norm_backward");
}
