// The depth convolution of the 3-d adapter (micro_sam/models/sam_3d_wrapper.py NDBlockWrapper: Conv3d(C, C, kernel_size=(3, 1, 1),
// padding="same")) on TOKEN-MAJOR data, as an implicit-shift GEMM:
//     out[b, z, t, :] = bias + sum_{j = 0..2} W_j x[b, z + j - 1, t, :]        (a term is dropped when z + j - 1 is outside [0, D))
// x: bf16 rows [B D T, Ci] (row m = (b D + z) T + t), W: bf16 [Co, 3 Ci] tap-major (columns j Ci .. (j + 1) Ci - 1 = tap j), out: fp32
// [B D T, Co].  It is the product A [M, 3 Ci] x W^T whose A row m is [x[m - T] | x[m] | x[m + T]] with the outer thirds zero at the
// ends of a volume - A is never written: the k-tile `kt` of tile row m is read from row m + (tap - 1) T of x, tap = kt / (Ci / 64).
//
// Tile body: the one of gemm.hip's gemm_body in its register-staging form - 128 x 128 x 64, 256 threads = 2 x 2 waves of 4 x 4
// v_mfma_f32_16x16x32_bf16, two LDS buffers with XOR-swizzled 128-B rows (common.h swz), global -> VGPR two k-tiles ahead -> ds_write,
// C staged through LDS for 16-byte stores.  The only new part is the A-side address: T need not divide the tile, so every staged row
// has its own slice index z = (m / T) % D and with it its own validity per tap.  A row that is not valid for the tap (or lies past M)
// is loaded from a LEGAL address - its own row m, clamped to M - 1 - and zeroed in registers before the LDS write; no address outside
// x is ever formed, also not for the first slice of the first volume and the last slice of the last one.
// No atomics; every output element is one fixed-order sum: two calls agree bit for bit.
#include "common.h"
#include <cstdio>
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int DC_BM = 128, DC_BN = 128, DC_BK = 64;
constexpr int DC_TILE_CHUNKS = DC_BM * 8;   // 16-B chunks per operand tile

MSAM_DEVINL uint4 dc_keep(const uint4& v, bool keep) {
    uint4 r;
    r.x = keep ? v.x : 0u; r.y = keep ? v.y : 0u; r.z = keep ? v.z : 0u; r.w = keep ? v.w : 0u;
    return r;
}

__global__ __launch_bounds__(256, 2) void depth_conv3_kernel(const u16* __restrict__ X, long ldx, const u16* __restrict__ W,
                                                             const float* __restrict__ bias, float* __restrict__ out, long ldc,
                                                             int M, int D, int T, int Ci, int Co) {
    __shared__ __attribute__((aligned(16))) uint4 lds[2][2][DC_TILE_CHUNKS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = Co / DC_BN, tiles_m = (M + DC_BM - 1) / DC_BM;
    // XCD-aware remap (bijective): consecutive tiles (sharing the A panel) run on one XCD / one L2
    int nwg = tiles_m * tiles_n, bid = (int)blockIdx.x;
    {
        int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
    const int m0 = tile_m * DC_BM, n0 = tile_n * DC_BN;
    const int wm = wave >> 1, wn = wave & 1;
    const long ldw = 3L * Ci;

    // staging map: thread t covers LDS chunk position (row = pass*32 + t/8, c' = t%8), which holds global chunk c' ^ swz(row).
    // aoff: byte offset of the row's OWN chunk in x (row clamped to M - 1); ok: bit j set = tap j of this row is inside its volume
    // (no bit for a row past M: all three thirds of such a row are zeros)
    const int srow = tid >> 3, scp = tid & 7;
    int aoff[4], woff[4], ok[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int row = p * 32 + srow;
        const int gc = scp ^ swz(row);
        const int m = m0 + row;
        const int ar = m > M - 1 ? M - 1 : m;
        const int z = (ar / T) % D;
        ok[p] = m < M ? ((z > 0 ? 1 : 0) | 2 | (z < D - 1 ? 4 : 0)) : 0;
        aoff[p] = (int)(((long)ar * ldx + gc * 8) * 2);
        woff[p] = (int)(((long)(n0 + row) * ldw + gc * 8) * 2);
    }
    const int shift = (int)((long)T * ldx * 2);            // bytes from a row to the same token one slice later

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int kpt = Ci / DC_BK;                            // k-tiles per tap
    const int nk = 3 * kpt;
    const int fr = lane & 15, fg = lane >> 4;
    auto compute = [&](int buf) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int row = wm * 64 + i * 16 + fr;
                a[i] = lds[buf][0][row * 8 + ((ks * 4 + fg) ^ swz(row))];
                int col = wn * 64 + i * 16 + fr;
                b[i] = lds[buf][1][col * 8 + ((ks * 4 + fg) ^ swz(col))];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        }
    };

    // the descriptors end with the last element the kernel may read: (M - 1) ldx + Ci of x, Co rows of W (the launcher keeps both
    // below 2^31 bytes, so the per-lane offsets are plain non-negative ints)
    const rsrc_t rx = make_rsrc(X, (uint32_t)((((long)M - 1) * ldx + Ci) * 2));
    const rsrc_t rw = make_rsrc(W, (uint32_t)((long)Co * ldw * 2));
    uint4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;          // first register set
    uint4 sa0, sa1, sa2, sa3, sw0, sw1, sw2, sw3;          // second register set
    // k-tile kt_: tap = kt_ / kpt (0, 1, 2), channels (kt_ % kpt) * 64 ... of that tap.  A valid row reads row m + (tap - 1) T, any
    // other row its own (legal) address; W reads its columns kt_ * 64 ... straight
#define DC_LOAD(a0_, a1_, a2_, a3_, w0_, w1_, w2_, w3_, kt_)                                           \
    do {                                                                                               \
        const int k__ = (kt_);                                                                         \
        const int tap__ = (k__ >= kpt ? 1 : 0) + (k__ >= 2 * kpt ? 1 : 0);                             \
        const int sh__ = (tap__ - 1) * shift;                                                          \
        const int sa__ = (k__ - tap__ * kpt) * DC_BK * 2, sw__ = k__ * DC_BK * 2;                      \
        a0_ = buf_load16(rx, aoff[0] + (((ok[0] >> tap__) & 1) ? sh__ : 0), sa__);                     \
        a1_ = buf_load16(rx, aoff[1] + (((ok[1] >> tap__) & 1) ? sh__ : 0), sa__);                     \
        a2_ = buf_load16(rx, aoff[2] + (((ok[2] >> tap__) & 1) ? sh__ : 0), sa__);                     \
        a3_ = buf_load16(rx, aoff[3] + (((ok[3] >> tap__) & 1) ? sh__ : 0), sa__);                     \
        w0_ = buf_load16(rw, woff[0], sw__); w1_ = buf_load16(rw, woff[1], sw__);                      \
        w2_ = buf_load16(rw, woff[2], sw__); w3_ = buf_load16(rw, woff[3], sw__);                      \
    } while (0)
    // kt_: the k-tile the registers were loaded for - rows that are not valid for its tap go to LDS as zeros
#define DC_COMMIT(a0_, a1_, a2_, a3_, w0_, w1_, w2_, w3_, buf_, kt_)                                   \
    do {                                                                                               \
        const int k__ = (kt_);                                                                         \
        const int tap__ = (k__ >= kpt ? 1 : 0) + (k__ >= 2 * kpt ? 1 : 0);                             \
        lds[buf_][0][(0 * 32 + srow) * 8 + scp] = dc_keep(a0_, (ok[0] >> tap__) & 1);                  \
        lds[buf_][0][(1 * 32 + srow) * 8 + scp] = dc_keep(a1_, (ok[1] >> tap__) & 1);                  \
        lds[buf_][0][(2 * 32 + srow) * 8 + scp] = dc_keep(a2_, (ok[2] >> tap__) & 1);                  \
        lds[buf_][0][(3 * 32 + srow) * 8 + scp] = dc_keep(a3_, (ok[3] >> tap__) & 1);                  \
        lds[buf_][1][(0 * 32 + srow) * 8 + scp] = w0_; lds[buf_][1][(1 * 32 + srow) * 8 + scp] = w1_;  \
        lds[buf_][1][(2 * 32 + srow) * 8 + scp] = w2_; lds[buf_][1][(3 * 32 + srow) * 8 + scp] = w3_;  \
    } while (0)
    // register staging TWO k-tiles ahead (two register sets, roles swapped by the 2x unrolled loop), as gemm.hip; nk >= 3 always
    DC_LOAD(ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3, 0);
    DC_COMMIT(ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3, 0, 0);
    DC_LOAD(ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3, 1);
    __syncthreads();
    int kt = 0;
    while (true) {
        DC_LOAD(sa0, sa1, sa2, sa3, sw0, sw1, sw2, sw3, min(kt + 2, nk - 1));
        compute(kt & 1);
        if (kt + 1 < nk) DC_COMMIT(ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3, (kt & 1) ^ 1, kt + 1);
        __syncthreads();
        if (++kt >= nk) break;
        DC_LOAD(ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3, min(kt + 2, nk - 1));
        compute(kt & 1);
        if (kt + 1 < nk) DC_COMMIT(sa0, sa1, sa2, sa3, sw0, sw1, sw2, sw3, (kt & 1) ^ 1, kt + 1);
        __syncthreads();
        if (++kt >= nk) break;
    }
    wait_vmem_all();                                       // the clamped tail prefetches must not outlive the LDS reuse below
#undef DC_LOAD
#undef DC_COMMIT

    // ---- epilogue: the fp32 C tile through LDS (the operand buffers), then 4 consecutive columns of one row per thread and pass
    float* ldsC = (float*)&lds[0][0][0];                   // [128][128] fp32 = 64 KB
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ldsC[(wm * 64 + i * 16 + fg * 4 + r) * DC_BN + wn * 64 + j * 16 + fr] = acc[i][j][r];
    __syncthreads();

    const int c4 = (tid & 31) * 4;
    const int col = n0 + c4;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) b4 = *(const float4*)(bias + col);
    const int lr0 = tid >> 5;
#pragma unroll
    for (int pass = 0; pass < 16; ++pass) {
        const int lr = pass * 8 + lr0;
        const int row = m0 + lr;
        if (row >= M) break;                               // rows only grow with pass; no barrier inside the loop
        const float4 c = *(const float4*)(ldsC + lr * DC_BN + c4);
        *(float4*)(out + (long)row * ldc + col) = make_float4(c.x + b4.x, c.y + b4.y, c.z + b4.z, c.w + b4.w);
    }
}

}  // namespace

extern "C" int msam_depth_conv3_bf16(const void* x, int64_t ldx, const void* w, const float* bias, float* out, int64_t ldc, int32_t B,
                                     int32_t D, int32_t T, int32_t Ci, int32_t Co, void* stream) {
    char msg[384];
    if (!x || !w || !out) { msam_set_error("msam_depth_conv3_bf16: null pointer"); return 1; }
    if (B < 1 || D < 1 || T < 1 || Ci < 64 || Co < 128 || Ci % 64 != 0 || Co % 128 != 0) {
        snprintf(msg, sizeof msg, "msam_depth_conv3_bf16: needs B, D, T >= 1, Ci a positive multiple of 64 and Co a positive multiple of "
                                  "128, got B = %d, D = %d, T = %d, Ci = %d, Co = %d", B, D, T, Ci, Co);
        msam_set_error(msg);
        return 1;
    }
    const int64_t M = (int64_t)B * D * T;
    if (ldx < Ci || ldc < Co || ldx % 8 != 0 || ldc % 4 != 0) {
        snprintf(msg, sizeof msg, "msam_depth_conv3_bf16: needs ldx >= Ci in eights and ldc >= Co in fours, got ldx = %lld, ldc = %lld",
                 (long long)ldx, (long long)ldc);
        msam_set_error(msg);
        return 1;
    }
    if (M >= (1LL << 31) || M * ldx * 2 >= (1LL << 31) || (int64_t)Co * 3 * Ci * 2 >= (1LL << 31) ||
        ((M + DC_BM - 1) / DC_BM) * (Co / DC_BN) >= (1LL << 31)) {
        snprintf(msg, sizeof msg, "msam_depth_conv3_bf16: x (B D T rows of ldx) and W must stay below 2^31 bytes each, got %lld rows of "
                                  "%lld", (long long)M, (long long)ldx);
        msam_set_error(msg);
        return 1;
    }
    if ((uintptr_t)x % 16 != 0 || (uintptr_t)w % 16 != 0 || (uintptr_t)out % 16 != 0 || (bias && (uintptr_t)bias % 16 != 0)) {
        msam_set_error("msam_depth_conv3_bf16: x, w, bias and out must be 16-byte aligned");
        return 1;
    }
    const unsigned tiles = (unsigned)(((M + DC_BM - 1) / DC_BM) * (Co / DC_BN));
    hipLaunchKernelGGL(depth_conv3_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const u16*)x, (long)ldx, (const u16*)w, bias,
                       out, (long)ldc, (int)M, (int)D, (int)T, (int)Ci, (int)Co);
    return msam_check_launch("msam_depth_conv3_bf16");
}
