// The AdaptFormer branch of an image-encoder block (models/peft_sam.py AdaptFormer; reference micro_sam/models/peft_sam.py AdaptFormer.forward)
// in one launch:
//     x[r, :] += y[r, :] + alpha * (relu(y[r, :] Wd^T + bd) Wu^T + bu)            y = norm2(x) in the encoder's 16-bit type, x the fp32 stream
// The block's MLP product adds `mlp(y)` to x on its own (encoder.hip); the `+ y` is the adapter's own "residual", which in the reference is
// the NORMED stream (the module's input), on top of the block's residual x.
//
// adapter_kernel<F16, PQ>, P = 32 PQ the bottleneck width.  A workgroup (256 threads, 2 x 2 waves) owns AD_BM = 32 rows.
//   Phase 1: hidden [32, P] = y [32, D] Wd^T over K = D in k-tiles of 64: y and Wd tiles in two LDS buffers each ([rows][64] 16-bit, 128-byte
//            rows, XOR swizzle common.h swz), global -> registers one k-tile ahead -> LDS, v_mfma_f32_16x16x32_{bf16,f16}; a wave holds 16 rows
//            x P / 2 columns.  Epilogue: + bd, ReLU, ONE rounding to the 16-bit type (the rounding site of the MLP hidden), written to LDS in the
//            A-operand layout: slabs of [32][64] (a slab of P = 32 or 96 is half used; the unused half is never read).
//   Phase 2: out [32, D] = hidden Wu^T in column chunks of 128 with K = P (P / 32 MFMA steps): the Wu chunk [128, P] is staged through the
//            buffers of phase 1 (one chunk ahead in registers); a wave holds 16 rows x 64 columns.  Epilogue straight from the accumulators:
//            x = x + fma(alpha, acc + bu, y) in fp32 - a lane quad-row writes 16 consecutive floats.
// The hidden never leaves LDS; alpha is read from device memory (a learnable scalar needs no host synchronisation).  Rows past R are loaded
// from row R - 1 (a legal address) and never stored.  No atomics, fixed summation order: two calls agree bit for bit.
#include "common.h"
#include <cstdio>
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int AD_BM = 32, AD_BK = 64, AD_BN = 128;

template <bool F16> MSAM_DEVINL f32x4_t ad_mfma(const uint4& a, const uint4& b, f32x4_t c) {
    if (F16) return mfma16h(a, b, c);
    return mfma16(a, b, c);
}
template <bool F16> MSAM_DEVINL u16 ad_round16(float v) { return F16 ? f2h(v) : f2bf(v); }
template <bool F16> MSAM_DEVINL float ad_to_f32(u16 v) { return F16 ? h2f(v) : bf2f(v); }

template <bool F16, int PQ>
__global__ __launch_bounds__(256) void adapter_kernel(const u16* __restrict__ Y, long ldy, const u16* __restrict__ Wd,
                                                      const float* __restrict__ bd, const u16* __restrict__ Wu,
                                                      const float* __restrict__ bu, const float* __restrict__ alpha, float* X, long ldx,
                                                      int R, int D) {
    constexpr int P = 32 * PQ;
    constexpr int PS = (P + 63) / 64;                      // 64-wide slabs of the hidden / of a Wu chunk
    constexpr int A_CH = AD_BM * 8;                        // 16-byte chunks of a y tile
    constexpr int W_CH = P * 8;                            // ... of a Wd tile
    constexpr int U_CH = PS * AD_BN * 8;                   // ... of a Wu chunk in slabs
    constexpr int STAGE = 2 * (A_CH + W_CH) > U_CH ? 2 * (A_CH + W_CH) : U_CH;
    constexpr int UP = AD_BN * PQ * 4 / 256;               // chunks of a Wu chunk per thread (P / 8 per row)
    __shared__ __attribute__((aligned(16))) uint4 stage[STAGE];         // phase 1: y buffers 0 / 1, Wd buffers 0 / 1; phase 2: the Wu chunk
    __shared__ __attribute__((aligned(16))) uint4 hid[PS * A_CH];       // the hidden, 16 bit, A-operand layout

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = (int)blockIdx.x * AD_BM;

    // ---- phase 1.  Staging map: thread t holds LDS chunk position (row = t / 8 (+ 32 p for Wd), c' = t % 8) = global chunk c' ^ swz(row)
    const int srow = tid >> 3, scp = tid & 7;
    const int arow = min(m0 + srow, R - 1);                // rows past R: a legal row, never stored
    const u16* ya = Y + (long)arow * ldy + (scp ^ swz(srow)) * 8;
    const u16* wa[PQ];
#pragma unroll
    for (int p = 0; p < PQ; ++p) {
        const int row = p * 32 + srow;
        wa[p] = Wd + (long)row * D + (scp ^ swz(row)) * 8;
    }
    f32x4_t acc[PQ];
#pragma unroll
    for (int j = 0; j < PQ; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nk = D / AD_BK;
    uint4 ra, rw[PQ];
    auto load1 = [&](int kt) {
        ra = *(const uint4*)(ya + kt * AD_BK);
#pragma unroll
        for (int p = 0; p < PQ; ++p) rw[p] = *(const uint4*)(wa[p] + kt * AD_BK);
    };
    auto commit1 = [&](int buf) {
        stage[buf * A_CH + srow * 8 + scp] = ra;
#pragma unroll
        for (int p = 0; p < PQ; ++p) stage[2 * A_CH + buf * W_CH + (p * 32 + srow) * 8 + scp] = rw[p];
    };
    load1(0);
    commit1(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load1(kt + 1);
        const uint4* la = stage + buf * A_CH;
        const uint4* lw = stage + 2 * A_CH + buf * W_CH;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int row = wm * 16 + fr;
            const uint4 a = la[row * 8 + ((ks * 4 + fg) ^ swz(row))];
#pragma unroll
            for (int j = 0; j < PQ; ++j) {
                const int col = (wn * PQ + j) * 16 + fr;
                const uint4 b = lw[col * 8 + ((ks * 4 + fg) ^ swz(col))];
                acc[j] = ad_mfma<F16>(a, b, acc[j]);
            }
        }
        if (kt + 1 < nk) commit1(buf ^ 1);                 // the other buffer: its last readers passed the barrier of the previous k-tile
        __syncthreads();
    }
    // hidden = round16(relu(acc + bd)), element (row, col) at slab col / 64, chunk ((col % 64) / 8) ^ swz(row)
    u16* hid16 = (u16*)hid;
#pragma unroll
    for (int j = 0; j < PQ; ++j) {
        const int col = (wn * PQ + j) * 16 + fr;
        const float b = bd[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wm * 16 + fg * 4 + r;
            const float h = relu1(__fadd_rn(acc[j][r], b));
            hid16[(col >> 6) * (A_CH * 8) + row * 64 + ((((col & 63) >> 3) ^ swz(row)) << 3) + (col & 7)] = ad_round16<F16>(h);
        }
    }

    // ---- phase 2.  Wu chunk [128, P]: thread t holds chunks q = p 256 + t: row = q / (P / 8), chunk c = q % (P / 8) of the row
    const float al = *alpha;
    uint4 ru[UP];
    auto load2 = [&](int n0) {
#pragma unroll
        for (int p = 0; p < UP; ++p) {
            const int q = p * 256 + tid;
            const int row = q / (PQ * 4), c = q % (PQ * 4);
            ru[p] = *(const uint4*)(Wu + (long)(n0 + row) * P + c * 8);
        }
    };
    auto commit2 = [&]() {
#pragma unroll
        for (int p = 0; p < UP; ++p) {
            const int q = p * 256 + tid;
            const int row = q / (PQ * 4), c = q % (PQ * 4);
            stage[(c >> 3) * (AD_BN * 8) + row * 8 + ((c & 7) ^ swz(row))] = ru[p];
        }
    };
    load2(0);
    commit2();                                             // (every wave left phase 1's buffers at the last barrier of its loop)
    __syncthreads();                                       // the hidden and the first Wu chunk are in place
    for (int n0 = 0; n0 < D; n0 += AD_BN) {
        if (n0 + AD_BN < D) load2(n0 + AD_BN);
        f32x4_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < PQ; ++ks) {
            const int row = wm * 16 + fr;
            const int ch = ((ks & 1) * 4 + fg);
            const uint4 a = hid[(ks >> 1) * A_CH + row * 8 + (ch ^ swz(row))];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = wn * 64 + j * 16 + fr;
                const uint4 b = stage[(ks >> 1) * (AD_BN * 8) + col * 8 + (ch ^ swz(col))];
                o[j] = ad_mfma<F16>(a, b, o[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + j * 16 + fr;
            const float b = bu[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 16 + fg * 4 + r;
                if (row < R) {
                    float* xp = X + (long)row * ldx + col;
                    const float yv = ad_to_f32<F16>(Y[(long)row * ldy + col]);
                    *xp = __fadd_rn(*xp, __fmaf_rn(al, __fadd_rn(o[j][r], b), yv));
                }
            }
        }
        __syncthreads();                                   // every wave is done with this chunk
        if (n0 + AD_BN < D) {
            commit2();
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int msam_adapter_bf16(const void* y16, int64_t ldy, const void* wd16, const float* bd, const void* wu16, const float* bu,
                                 const float* alpha, float* x, int64_t ldx, int32_t R, int32_t D, int32_t P, int32_t dtype16,
                                 void* stream) {
    char msg[384];
    if (!y16 || !wd16 || !bd || !wu16 || !bu || !alpha || !x) { msam_set_error("msam_adapter_bf16: null pointer"); return 1; }
    if (R < 1 || D < 128 || D % 128 != 0 || P < 32 || P > 128 || P % 32 != 0 || (dtype16 != MSAM_BF16 && dtype16 != MSAM_F16)) {
        snprintf(msg, sizeof msg, "msam_adapter_bf16: needs R >= 1, D a positive multiple of 128, P a multiple of 32 in 32 .. 128 and dtype16 "
                                  "MSAM_BF16 or MSAM_F16, got R = %d, D = %d, P = %d, dtype16 = %d", R, D, P, dtype16);
        msam_set_error(msg);
        return 1;
    }
    if (ldy < D || ldy % 8 != 0 || ldx < D) {
        snprintf(msg, sizeof msg, "msam_adapter_bf16: needs ldy >= D in eights and ldx >= D, got ldy = %lld, ldx = %lld", (long long)ldy,
                 (long long)ldx);
        msam_set_error(msg);
        return 1;
    }
    if ((uintptr_t)y16 % 16 != 0 || (uintptr_t)wd16 % 16 != 0 || (uintptr_t)wu16 % 16 != 0 || (uintptr_t)x % 4 != 0 ||
        (uintptr_t)bd % 4 != 0 || (uintptr_t)bu % 4 != 0 || (uintptr_t)alpha % 4 != 0) {
        msam_set_error("msam_adapter_bf16: y16, wd16 and wu16 must be 16-byte aligned, the fp32 operands 4-byte aligned");
        return 1;
    }
    const unsigned tiles = (unsigned)(((int64_t)R + AD_BM - 1) / AD_BM);
#define AD_LAUNCH(F16_, PQ_)                                                                                                         \
    hipLaunchKernelGGL((adapter_kernel<F16_, PQ_>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const u16*)y16, (long)ldy,      \
                       (const u16*)wd16, bd, (const u16*)wu16, bu, alpha, x, (long)ldx, (int)R, (int)D)
    const int pq = P / 32;
    if (dtype16 == MSAM_F16) {
        if (pq == 1) AD_LAUNCH(true, 1); else if (pq == 2) AD_LAUNCH(true, 2); else if (pq == 3) AD_LAUNCH(true, 3); else AD_LAUNCH(true, 4);
    } else {
        if (pq == 1) AD_LAUNCH(false, 1); else if (pq == 2) AD_LAUNCH(false, 2); else if (pq == 3) AD_LAUNCH(false, 3); else AD_LAUNCH(false, 4);
    }
#undef AD_LAUNCH
    return msam_check_launch("msam_adapter_bf16");
}
