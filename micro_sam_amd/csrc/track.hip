// Device side of tracking many objects through a time series (tracking.track_objects_in_timeseries; reference
// micro_sam/sam_annotator/util.py:561-579 _compute_movement / _shift_object inside track_from_prompts :582-675): the two steps the
// slice-to-slice propagation of csrc/propagate.hip lacks - the centre of a bit mask and its shift by a per-object sub-pixel motion.
//
// Layout of every mask stack: uint32 [P, ceil(H / 32), W], bit b of word [p][yw][x] = pixel (yw * 32 + b, x), as in propagate.hip.
// Bits of rows >= H in the last word row of an INPUT are ignored and may hold anything; the same bits of an OUTPUT are zero.
//
//   moments : out int64 [P, 3] = (count, sum of y, sum of x) over the set pixels, exact.  Per word: the count is a popcount, the sum of
//             x is x * popcount, the sum of the bit positions is five masked popcounts (bit k of the position is set in the bits of
//             TK_POS[k]).  64-bit accumulators per lane (the sum of y of a full 2049 x 2049 mask is already above 2^32), wave reduction
//             of the two halves, LDS across the four waves, three 64-bit integer atomics per workgroup.  The division is the host's.
//   shift   : out(y, x) = in(src_y(y), src_x(x)), zero where either source is invalid; per axis of length n and shift s, every step
//             its own fp64 rounding,
//                 cc = (double)i - s;   valid = cc >= 0 && cc <= n - 1;   src = (int)floor(cc + 0.5)
//             which is scipy.ndimage.shift(mask, (sy, sx), order=0, prefilter=False), mode "constant", cval 0.  src(i) - i is NOT one
//             integer per axis (where s lies within rounding of k + 1/2 it changes along the axis), so the rule is evaluated per index:
//             one lane per output word (consecutive lanes = consecutive x: coalesced), its own src_x in a register, the 32 src_y of the
//             workgroup's word row in LDS.  Where the 32 rows have consecutive valid sources the word is funnel-shifted out of two input
//             words; every other word gathers bit by bit (re-reading a word only when the source word row changes).
//
// Integer sums and integer atomics only: two runs give the same bits.  No workspace, no allocation, no synchronisation.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

MSAM_DEVINL unsigned tk_tail_mask(int H, int yw) {                     // the bits of word row yw that are rows of the image
    const int left = H - yw * 32;
    return left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
}

MSAM_DEVINL unsigned long long tk_wave_add(unsigned long long v) {     // the two halves travel apart and are put together again
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(256) void tk_zero_kernel(int n, unsigned long long* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0ull;
}

// grid (min(ceil(WPC * W / 256), 64), P): the words of one object are strided over its workgroups
__global__ __launch_bounds__(256) void tk_moments_kernel(const unsigned* __restrict__ bits, int H, int W, int WPC,
                                                         unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[3][4];
    const int p = blockIdx.y, n = WPC * W;
    const unsigned* __restrict__ src = bits + (size_t)p * n;
    const unsigned tm = tk_tail_mask(H, WPC - 1);
    unsigned long long cnt = 0, sy = 0, sx = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int yw = i / W, x = i - yw * W;
        const unsigned w = src[i] & (yw == WPC - 1 ? tm : 0xffffffffu);
        if (!w) continue;
        const int c = __popc(w);
        const int pos = __popc(w & 0xaaaaaaaau) + 2 * __popc(w & 0xccccccccu) + 4 * __popc(w & 0xf0f0f0f0u) +
                        8 * __popc(w & 0xff00ff00u) + 16 * __popc(w & 0xffff0000u);      // sum of the positions of the set bits
        cnt += (unsigned long long)c;
        sy += (unsigned long long)((long long)yw * 32 * c + pos);
        sx += (unsigned long long)((long long)x * c);
    }
    cnt = tk_wave_add(cnt);
    sy = tk_wave_add(sy);
    sx = tk_wave_add(sx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = cnt; part[1][wave] = sy; part[2][wave] = sx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        if (cnt) {
            atomicAdd(&out[3 * p], cnt);
            atomicAdd(&out[3 * p + 1], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
            atomicAdd(&out[3 * p + 2], part[2][0] + part[2][1] + part[2][2] + part[2][3]);
        }
    }
}

// source index of output index i on an axis of length n under the shift s, -1 where the output is the constant 0.  Every comparison
// with a NaN is false, so a NaN shift (and an infinite one) leaves nothing valid.  A subtraction, an addition: nothing to contract.
MSAM_DEVINL int tk_source(int i, int n, double s) {
    const double cc = (double)i - s;
    if (!(cc >= 0.0 && cc <= (double)(n - 1))) return -1;
    return (int)floor(cc + 0.5);                                       // in [0, n - 1]: cc + 0.5 <= n - 0.5
}

// grid (ceil(W / 256) * WPC, P): one lane per output word; the workgroup shares a word row
__global__ __launch_bounds__(256) void tk_shift_kernel(const unsigned* __restrict__ in, int H, int W, int WPC, int XB,
                                                       const double* __restrict__ shifts, unsigned* __restrict__ out) {
    __shared__ int rows[32];
    const int p = blockIdx.y, yw = blockIdx.x / XB, x = (blockIdx.x - yw * XB) * 256 + threadIdx.x;
    if (threadIdx.x < 32) {
        const int y = yw * 32 + threadIdx.x;
        rows[threadIdx.x] = y < H ? tk_source(y, H, shifts[2 * p]) : -1;             // rows past the image: the zero tail of the output
    }
    __syncthreads();
    if (x >= W) return;
    const int sx = tk_source(x, W, shifts[2 * p + 1]);
    unsigned word = 0;
    if (sx >= 0) {
        const unsigned* __restrict__ col = in + (size_t)p * WPC * W + sx;
        const int s0 = rows[0];
        bool run = s0 >= 0;                                            // the 32 rows read 32 consecutive rows of the input
#pragma unroll
        for (int b = 1; b < 32; ++b) run = run && rows[b] == s0 + b;
        if (run) {
            // s0 + 31 <= H - 1: every row read is a row of the image (no tail bit of the input gets in), and for r != 0 the word row
            // q + 1 = (s0 + 31) >> 5 exists
            const int q = s0 >> 5, r = s0 & 31;
            const unsigned lo = col[(size_t)q * W];
            word = r ? (lo >> r) | (col[(size_t)(q + 1) * W] << (32 - r)) : lo;      // (a shift by 32 is undefined: r = 0 apart)
        } else {
            int have = -1;
            unsigned w = 0;
#pragma unroll
            for (int b = 0; b < 32; ++b) {
                const int s = rows[b];                                 // in [0, H - 1] or -1: never a tail bit of the input
                if (s < 0) continue;
                if ((s >> 5) != have) { have = s >> 5; w = col[(size_t)have * W]; }
                word |= ((w >> (s & 31)) & 1u) << b;
            }
        }
    }
    out[((size_t)p * WPC + yw) * W + x] = word;
}

bool tk_shape_ok(int32_t P, int32_t H, int32_t W) {
    return P >= 1 && P <= MSAM_MASK_MAX_OBJECTS && H >= 1 && W >= 1 && H <= MSAM_MASK_MAX_SIDE && W <= MSAM_MASK_MAX_SIDE;
}

#define TK_SHAPE_MSG ": 1 <= P <= 65535 and 1 <= H, W <= 32767"

}  // namespace

extern "C" int msam_mask_moments(const uint32_t* bits, int32_t P, int32_t H, int32_t W, int64_t* out, void* stream) {
    if (!bits || !out) { msam_set_error("msam_mask_moments: null pointer"); return 1; }
    if (!tk_shape_ok(P, H, W)) { msam_set_error("msam_mask_moments" TK_SHAPE_MSG); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const int WPC = (H + 31) / 32;
    const int64_t blocks = ((int64_t)WPC * W + 255) / 256;
    unsigned long long* acc = (unsigned long long*)out;                // non-negative sums below 2^63: the same bits as int64
    hipLaunchKernelGGL(tk_zero_kernel, dim3((unsigned)((3 * P + 255) / 256)), dim3(256), 0, s, 3 * P, acc);
    hipLaunchKernelGGL(tk_moments_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), (unsigned)P), dim3(256), 0, s, bits, H, W, WPC, acc);
    return msam_check_launch("msam_mask_moments");
}

extern "C" int msam_mask_shift(const uint32_t* bits_in, int32_t P, int32_t H, int32_t W, const double* shifts, uint32_t* bits_out,
                               void* stream) {
    if (!bits_in || !shifts || !bits_out) { msam_set_error("msam_mask_shift: null pointer"); return 1; }
    if (!tk_shape_ok(P, H, W)) { msam_set_error("msam_mask_shift" TK_SHAPE_MSG); return 1; }
    if (bits_in == bits_out) { msam_set_error("msam_mask_shift: bits_out must not be bits_in (a lane reads words other lanes write)"); return 1; }
    const int WPC = (H + 31) / 32, XB = (W + 255) / 256;
    hipLaunchKernelGGL(tk_shift_kernel, dim3((unsigned)(XB * WPC), (unsigned)P), dim3(256), 0, (hipStream_t)stream, bits_in, H, W, WPC, XB,
                       shifts, bits_out);
    return msam_check_launch("msam_mask_shift");
}
