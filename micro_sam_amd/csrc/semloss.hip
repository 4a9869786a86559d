// Device side of micro_sam_amd.training.semantic_sam_trainer: the loss of semantic-segmentation fine-tuning (reference
// micro_sam/training/semantic_sam_trainer.py: CustomDiceLoss, i.e. torch_em's DiceLoss on a soft-max and a one-hot target, plus
// nn.CrossEntropyLoss) on logits float32 [B, C, HW] (every class its own plane per image) and class ids int32 [B, HW], 2 <= C <= 32.
//
//   p = softmax_c(logits) per pixel (or p = logits), t_c = [target == c]; a pixel is VALID when 0 <= target < C, every other id (torch's
//   ignore_index -100 among them) has an all-zero one-hot and does not count in the cross-entropy.
//   dice = sum_c (1 - 2 num_c / max(den_c, eps)),  num_c = sum p_c t_c,  den_c = sum p_c^2 + sum t_c    (sums over all B * HW pixels)
//   ce   = sum_valid (logsumexp(logits) - logits[target]) / n_valid                                      (0 when no pixel is valid)
//   loss = dice_weight * dice + ce_weight * ce
//
//   forward  : sl_sums_kernel - a workgroup owns 2048 consecutive pixels, 8 per thread (two float4 / int4 loads per plane where HW % 4 == 0
//              and the pointers are 16-byte aligned, eight one-pixel loads otherwise); exp and log in fp32, the soft-max division and every sum in fp64
//              (no fp32 sum at all); the 2 C + 1 sums and C + 2 counts of a thread go through a xor butterfly over the wave, the four waves
//              are added in index order through LDS and the workgroup writes its partials to the workspace.  sl_finish_kernel, ONE
//              workgroup: thread i adds the partials i, i + 256, ... in index order, the same butterfly and wave order, then thread 0
//              forms the loss and the statistics.  Which pixel goes to which thread and workgroup depends on the shape (and the alignment
//              class) alone, so two calls agree bit for bit.
//   backward : sl_backward_kernel, one elementwise pass that recomputes p (the statistics give num_c, den_c and n_valid):
//              g_c = dice_weight * [den_c > eps] * (-2 t_c / d_c + 4 num_c p_c / d_c^2),  d_c = max(den_c, eps)
//              dlogits_k = (p_k (g_k - sum_c p_c g_c) + ce_weight * valid * (p_k - t_k) / n_valid) * upstream    (dlogits = g without soft-max)
//              in fp64 from the fp32 p, rounded once.  The upstream gradient is read on the device.
//   C <= 8 keeps the logits of a pixel in registers (sl_*_kernel<CT, NP>, CT = 2, 3, 4, 8); above, run-time loops over the classes read
//   the planes again (sl_*_rt_kernel: twice in the forward pass, three times in the backward pass).
// No floating-point atomics, plain vector / C++ stores, caller-provided workspace, no host synchronisation.
#include "common.h"
#include <cstdio>
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

constexpr int SL_PIX = 2048;                                             // pixels per workgroup: 8 per thread
constexpr int SL_MAXC = MSAM_SEMLOSS_MAX_CLASSES;

MSAM_DEVINL double sl_shfl_xor(double v, int o) {                        // (two 32-bit exchanges: also what the host build of the tests has)
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
    const int lo = __shfl_xor((int)(unsigned)b, o), hi = __shfl_xor((int)(unsigned)(b >> 32), o);
    b = ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
    __builtin_memcpy(&v, &b, 8);
    return v;
}
MSAM_DEVINL double sl_wave_sum(double v) {
    v += sl_shfl_xor(v, 1); v += sl_shfl_xor(v, 2); v += sl_shfl_xor(v, 4);
    v += sl_shfl_xor(v, 8); v += sl_shfl_xor(v, 16); v += sl_shfl_xor(v, 32);
    return v;
}
MSAM_DEVINL int sl_wave_sum(int v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    return v;
}

template <int NP> MSAM_DEVINL void sl_load(const float* __restrict__ p, float (&v)[NP]) {
    if constexpr (NP == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}
template <int NP> MSAM_DEVINL void sl_load(const int32_t* __restrict__ p, int (&v)[NP]) {
    if constexpr (NP == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = (int)q.x; v[1] = (int)q.y; v[2] = (int)q.z; v[3] = (int)q.w;
    } else {
        v[0] = *p;
    }
}
template <int NP> MSAM_DEVINL void sl_store(float* __restrict__ p, const float (&v)[NP]) {
    if constexpr (NP == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// unit `it` of this thread: NP consecutive pixels of one image -> offset of the pixel in the target, of its class-0 logit in the logits
template <int NP> MSAM_DEVINL bool sl_unit(int it, int C, int HW, long total, long* toff, long* loff) {
    const long unit = (long)blockIdx.x * (SL_PIX / NP) + (long)it * 256 + threadIdx.x;
    const long pix = unit * NP;
    if (pix >= total) return false;                                      // (NP == 4: total is a multiple of 4)
    const long b = pix / HW, i = pix - b * HW;
    *toff = pix;
    *loff = b * C * (long)HW + i;
    return true;
}

// the partials of a workgroup: lane 0 of every wave has left its sums in smD / smI; the four waves in index order
MSAM_DEVINL void sl_write_partials(double (*smD)[2 * SL_MAXC + 1], int (*smI)[SL_MAXC + 2], int C, double* __restrict__ partD,
                                   int* __restrict__ partI) {
    const int QD = 2 * C + 1, QI = C + 2, tid = threadIdx.x;
    __syncthreads();
    if (tid < QD) partD[(size_t)blockIdx.x * QD + tid] = ((smD[0][tid] + smD[1][tid]) + smD[2][tid]) + smD[3][tid];
    if (tid < QI) partI[(size_t)blockIdx.x * QI + tid] = ((smI[0][tid] + smI[1][tid]) + smI[2][tid]) + smI[3][tid];
}

// grid (ceil(total / 2048)); partD [nwg, 2 C + 1] = num_c, sum p_c^2, the cross-entropy sum; partI [nwg, C + 2] = sum t_c, valid, ignored
template <int CT, int NP>
__global__ __launch_bounds__(256) void sl_sums_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, int C, int HW,
                                                      long total, int softmax, double* __restrict__ partD, int* __restrict__ partI) {
    __shared__ double smD[4][2 * SL_MAXC + 1];
    __shared__ int smI[4][SL_MAXC + 2];
    double num[CT], psq[CT], ce = 0.0;
    int cnt[CT], nvalid = 0, nign = 0;
#pragma unroll
    for (int c = 0; c < CT; ++c) { num[c] = 0.0; psq[c] = 0.0; cnt[c] = 0; }
#pragma unroll
    for (int it = 0; it < 8 / NP; ++it) {
        long toff, loff;
        if (!sl_unit<NP>(it, C, HW, total, &toff, &loff)) continue;
        int t[NP];
        float x[CT][NP];
        sl_load<NP>(target + toff, t);
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) sl_load<NP>(logits + loff + (long)c * HW, x[c]);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const bool valid = t[j] >= 0 && t[j] < C;
            nvalid += valid; nign += !valid;
            double p[CT];
            if (softmax) {
                float m = x[0][j];
#pragma unroll
                for (int c = 1; c < CT; ++c)
                    if (c < C) m = fmaxf(m, x[c][j]);
                float e[CT], xt = m;
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) {
                        e[c] = expf(__fsub_rn(x[c][j], m));
                        s += (double)e[c];
                        if (c == t[j]) xt = x[c][j];
                    }
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) p[c] = (double)e[c] / s;
                if (valid) ce += (double)logf((float)s) - ((double)xt - (double)m);
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) p[c] = (double)x[c][j];
            }
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < C) {
                    psq[c] += p[c] * p[c];
                    if (c == t[j]) { num[c] += p[c]; cnt[c] += 1; }
                }
        }
    }
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < CT; ++c)
        if (c < C) {                                                     // (uniform)
            const double a = sl_wave_sum(num[c]), b = sl_wave_sum(psq[c]);
            const int n = sl_wave_sum(cnt[c]);
            if (l == 0) { smD[w][c] = a; smD[w][C + c] = b; smI[w][c] = n; }
        }
    ce = sl_wave_sum(ce); nvalid = sl_wave_sum(nvalid); nign = sl_wave_sum(nign);
    if (l == 0) { smD[w][2 * C] = ce; smI[w][C] = nvalid; smI[w][C + 1] = nign; }
    sl_write_partials(smD, smI, C, partD, partI);
}

// the same for 8 < C <= 32: pass 1 finds the maximum and the sum of exponentials of the thread's 8 pixels (online), pass 2 reads the
// planes again class by class and reduces each class's three sums at once
template <int NP>
__global__ __launch_bounds__(256) void sl_sums_rt_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, int C, int HW,
                                                         long total, int softmax, double* __restrict__ partD, int* __restrict__ partI) {
    __shared__ double smD[4][2 * SL_MAXC + 1];
    __shared__ int smI[4][SL_MAXC + 2];
    constexpr int IT = 8 / NP;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    long loff[IT];
    bool live[IT];
    int t[IT][NP];
    float m[IT][NP];
    double s[IT][NP], ce = 0.0;
    int nvalid = 0, nign = 0;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        long toff;
        live[it] = sl_unit<NP>(it, C, HW, total, &toff, &loff[it]);
#pragma unroll
        for (int j = 0; j < NP; ++j) { t[it][j] = -1; m[it][j] = 0.f; s[it][j] = 1.0; }
        if (!live[it]) continue;
        sl_load<NP>(target + toff, t[it]);
        float xt[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const bool valid = t[it][j] >= 0 && t[it][j] < C;
            nvalid += valid; nign += !valid;
            xt[j] = 0.f;
        }
        if (!softmax) continue;
        for (int c = 0; c < C; ++c) {
            float x[NP];
            sl_load<NP>(logits + loff[it] + (long)c * HW, x);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                if (c == 0) { m[it][j] = x[j]; s[it][j] = 1.0; }
                else if (x[j] > m[it][j]) { s[it][j] = s[it][j] * (double)expf(__fsub_rn(m[it][j], x[j])) + 1.0; m[it][j] = x[j]; }
                else s[it][j] += (double)expf(__fsub_rn(x[j], m[it][j]));
                if (c == t[it][j]) xt[j] = x[j];
            }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (t[it][j] >= 0 && t[it][j] < C) ce += (double)logf((float)s[it][j]) - ((double)xt[j] - (double)m[it][j]);
    }
    for (int c = 0; c < C; ++c) {
        double num = 0.0, psq = 0.0;
        int cnt = 0;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            if (!live[it]) continue;
            float x[NP];
            sl_load<NP>(logits + loff[it] + (long)c * HW, x);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const double p = softmax ? (double)expf(__fsub_rn(x[j], m[it][j])) / s[it][j] : (double)x[j];
                psq += p * p;
                if (c == t[it][j]) { num += p; cnt += 1; }
            }
        }
        num = sl_wave_sum(num); psq = sl_wave_sum(psq); cnt = sl_wave_sum(cnt);
        if (l == 0) { smD[w][c] = num; smD[w][C + c] = psq; smI[w][c] = cnt; }
    }
    ce = sl_wave_sum(ce); nvalid = sl_wave_sum(nvalid); nign = sl_wave_sum(nign);
    if (l == 0) { smD[w][2 * C] = ce; smI[w][C] = nvalid; smI[w][C + 1] = nign; }
    sl_write_partials(smD, smI, C, partD, partI);
}

// ONE workgroup.  statsD [2 C + 3] = num_c, sum p_c^2, the cross-entropy sum, dice, ce; statsI [C + 2] = sum t_c, valid, ignored
__global__ __launch_bounds__(256) void sl_finish_kernel(const double* __restrict__ partD, const int* __restrict__ partI, int nwg, int C,
                                                        float dice_weight, float ce_weight, int softmax, double eps, float* __restrict__ loss,
                                                        double* __restrict__ statsD, long long* __restrict__ statsI) {
    __shared__ double smD[4][2 * SL_MAXC + 1];
    __shared__ long long smI[4][SL_MAXC + 2];
    const int QD = 2 * C + 1, QI = C + 2, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    for (int q = 0; q < QD; ++q) {
        double s = 0.0;
        for (int g = tid; g < nwg; g += 256) s += partD[(size_t)g * QD + q];
        s = sl_wave_sum(s);
        if (l == 0) smD[w][q] = s;
    }
    for (int q = 0; q < QI; ++q) {
        int s = 0;                                                       // (at most 2^31 - 1 pixels in all)
        for (int g = tid; g < nwg; g += 256) s += partI[(size_t)g * QI + q];
        s = sl_wave_sum(s);
        if (l == 0) smI[w][q] = s;
    }
    __syncthreads();
    if (tid < QD) statsD[tid] = ((smD[0][tid] + smD[1][tid]) + smD[2][tid]) + smD[3][tid];
    if (tid < QI) statsI[tid] = ((smI[0][tid] + smI[1][tid]) + smI[2][tid]) + smI[3][tid];
    __syncthreads();
    if (tid == 0) {
        double dice = 0.0;
        for (int c = 0; c < C; ++c) {
            const double den = statsD[C + c] + (double)statsI[c];
            dice += 1.0 - 2.0 * statsD[c] / (den > eps ? den : eps);
        }
        const long long nvalid = statsI[C];
        const double ce = (softmax && nvalid > 0) ? statsD[2 * C] / (double)nvalid : 0.0;
        statsD[2 * C + 1] = dice;
        statsD[2 * C + 2] = ce;
        *loss = (float)((double)dice_weight * dice + (double)ce_weight * ce);
    }
}

// the coefficients of the backward pass from the statistics: g_c = ga[c] t_c + gb[c] p_c; cen = ce_weight / n_valid
MSAM_DEVINL void sl_coefficients(const double* __restrict__ statsD, const long long* __restrict__ statsI, int C, float dice_weight,
                                 float ce_weight, int softmax, double eps, double* ga, double* gb, double* cen) {
    const int tid = threadIdx.x;
    if (tid < C) {
        const double den = statsD[C + tid] + (double)statsI[tid];
        const bool live = den > eps;
        const double d = live ? den : eps;
        ga[tid] = live ? -2.0 * (double)dice_weight / d : 0.0;
        gb[tid] = live ? 4.0 * (double)dice_weight * statsD[tid] / (d * d) : 0.0;
    }
    if (tid == 0) {
        const long long nvalid = statsI[C];
        *cen = (softmax && nvalid > 0) ? (double)ce_weight / (double)nvalid : 0.0;
    }
    __syncthreads();
}

template <int CT, int NP>
__global__ __launch_bounds__(256) void sl_backward_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, int C, int HW,
                                                          long total, float dice_weight, float ce_weight, int softmax, double eps,
                                                          const double* __restrict__ statsD, const long long* __restrict__ statsI,
                                                          const float* __restrict__ grad_out, float* __restrict__ dlogits) {
    __shared__ double ga[SL_MAXC], gb[SL_MAXC], cen;
    sl_coefficients(statsD, statsI, C, dice_weight, ce_weight, softmax, eps, ga, gb, &cen);
    const double up = (double)*grad_out;
#pragma unroll
    for (int it = 0; it < 8 / NP; ++it) {
        long toff, loff;
        if (!sl_unit<NP>(it, C, HW, total, &toff, &loff)) continue;
        int t[NP];
        float x[CT][NP], out[CT][NP];
        sl_load<NP>(target + toff, t);
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) sl_load<NP>(logits + loff + (long)c * HW, x[c]);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const bool valid = t[j] >= 0 && t[j] < C;
            double p[CT], g[CT];
            if (softmax) {
                float m = x[0][j];
#pragma unroll
                for (int c = 1; c < CT; ++c)
                    if (c < C) m = fmaxf(m, x[c][j]);
                float e[CT];
                double s = 0.0, dot = 0.0;
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) { e[c] = expf(__fsub_rn(x[c][j], m)); s += (double)e[c]; }
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) {
                        p[c] = (double)e[c] / s;
                        g[c] = gb[c] * p[c] + (c == t[j] ? ga[c] : 0.0);
                        dot += p[c] * g[c];
                    }
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) {
                        const double ce = valid ? cen * (p[c] - (c == t[j] ? 1.0 : 0.0)) : 0.0;
                        out[c][j] = (float)((p[c] * (g[c] - dot) + ce) * up);
                    }
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (c < C) out[c][j] = (float)((gb[c] * (double)x[c][j] + (c == t[j] ? ga[c] : 0.0)) * up);
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) sl_store<NP>(dlogits + loff + (long)c * HW, out[c]);
    }
}

template <int NP>
__global__ __launch_bounds__(256) void sl_backward_rt_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, int C, int HW,
                                                             long total, float dice_weight, float ce_weight, int softmax, double eps,
                                                             const double* __restrict__ statsD, const long long* __restrict__ statsI,
                                                             const float* __restrict__ grad_out, float* __restrict__ dlogits) {
    __shared__ double ga[SL_MAXC], gb[SL_MAXC], cen;
    sl_coefficients(statsD, statsI, C, dice_weight, ce_weight, softmax, eps, ga, gb, &cen);
    const double up = (double)*grad_out;
    for (int it = 0; it < 8 / NP; ++it) {
        long toff, loff;
        if (!sl_unit<NP>(it, C, HW, total, &toff, &loff)) continue;
        int t[NP];
        sl_load<NP>(target + toff, t);
        float m[NP];
        double s[NP], dot[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) { m[j] = 0.f; s[j] = 1.0; dot[j] = 0.0; }
        if (softmax) {
            for (int c = 0; c < C; ++c) {
                float x[NP];
                sl_load<NP>(logits + loff + (long)c * HW, x);
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    if (c == 0) { m[j] = x[j]; s[j] = 1.0; }
                    else if (x[j] > m[j]) { s[j] = s[j] * (double)expf(__fsub_rn(m[j], x[j])) + 1.0; m[j] = x[j]; }
                    else s[j] += (double)expf(__fsub_rn(x[j], m[j]));
                }
            }
            for (int c = 0; c < C; ++c) {
                float x[NP];
                sl_load<NP>(logits + loff + (long)c * HW, x);
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const double p = (double)expf(__fsub_rn(x[j], m[j])) / s[j];
                    dot[j] += p * (gb[c] * p + (c == t[j] ? ga[c] : 0.0));
                }
            }
        }
        for (int c = 0; c < C; ++c) {
            float x[NP], out[NP];
            sl_load<NP>(logits + loff + (long)c * HW, x);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const double a = c == t[j] ? ga[c] : 0.0;
                if (softmax) {
                    const bool valid = t[j] >= 0 && t[j] < C;
                    const double p = (double)expf(__fsub_rn(x[j], m[j])) / s[j];
                    const double ce = valid ? cen * (p - (c == t[j] ? 1.0 : 0.0)) : 0.0;
                    out[j] = (float)((p * ((gb[c] * p + a) - dot[j]) + ce) * up);
                } else {
                    out[j] = (float)((gb[c] * (double)x[j] + a) * up);
                }
            }
            sl_store<NP>(dlogits + loff + (long)c * HW, out);
        }
    }
}

bool sl_shape_ok(int32_t B, int32_t C, int32_t HW) {
    return B >= 1 && C >= 2 && C <= SL_MAXC && HW >= 1 && (int64_t)B * C * HW < (1ll << 31);
}

const char* const SL_SHAPE = "B >= 1 images of 2 <= C <= 32 classes and HW >= 1 pixels with B * C * HW < 2^31";

bool sl_weights_ok(float dice_weight, float ce_weight, int32_t apply_softmax, double eps) {
    return (apply_softmax == 0 || apply_softmax == 1) && (apply_softmax == 1 || ce_weight == 0.f) && dice_weight == dice_weight &&
           ce_weight == ce_weight && eps > 0.0;
}

const char* const SL_WEIGHTS = "apply_softmax is 0 or 1, the cross-entropy needs the soft-max (ce_weight must be 0 without it), the weights are "
                               "numbers and eps > 0";

inline bool sl_vec(int32_t HW, const void* a, const void* b, const void* c) {
    return HW % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && (uintptr_t)c % 16 == 0;
}

}  // namespace

extern "C" int64_t msam_semantic_loss_workspace_bytes(int32_t B, int32_t C, int32_t HW) {
    if (!sl_shape_ok(B, C, HW)) return 0;
    const int64_t nwg = ((int64_t)B * HW + SL_PIX - 1) / SL_PIX;
    return nwg * (2 * C + 1) * 8 + (nwg * (C + 2) * 4 + 7) / 8 * 8;
}

#define SL_LAUNCH(kern_, rt_, ...)                                                                                            \
    do {                                                                                                                      \
        if (C == 2) hipLaunchKernelGGL((kern_<2, NP>), dim3((unsigned)nwg), dim3(256), 0, s, __VA_ARGS__);                    \
        else if (C == 3) hipLaunchKernelGGL((kern_<3, NP>), dim3((unsigned)nwg), dim3(256), 0, s, __VA_ARGS__);               \
        else if (C == 4) hipLaunchKernelGGL((kern_<4, NP>), dim3((unsigned)nwg), dim3(256), 0, s, __VA_ARGS__);               \
        else if (C <= 8) hipLaunchKernelGGL((kern_<8, NP>), dim3((unsigned)nwg), dim3(256), 0, s, __VA_ARGS__);               \
        else hipLaunchKernelGGL((rt_<NP>), dim3((unsigned)nwg), dim3(256), 0, s, __VA_ARGS__);                                \
    } while (0)

namespace {

template <int NP>
void sl_launch_sums(unsigned nwg, hipStream_t s, const float* logits, const int32_t* target, int C, int HW, long total, int softmax,
                    double* partD, int* partI) {
    SL_LAUNCH(sl_sums_kernel, sl_sums_rt_kernel, logits, target, C, HW, total, softmax, partD, partI);
}

template <int NP>
void sl_launch_backward(unsigned nwg, hipStream_t s, const float* logits, const int32_t* target, int C, int HW, long total, float dice_weight,
                        float ce_weight, int softmax, double eps, const double* statsD, const long long* statsI, const float* grad_out,
                        float* dlogits) {
    SL_LAUNCH(sl_backward_kernel, sl_backward_rt_kernel, logits, target, C, HW, total, dice_weight, ce_weight, softmax, eps, statsD, statsI,
              grad_out, dlogits);
}

}  // namespace

extern "C" int msam_semantic_loss_forward(const float* logits, const int32_t* target, int32_t B, int32_t C, int32_t HW, float dice_weight,
                                          float ce_weight, int32_t apply_softmax, double eps, void* workspace, int64_t workspace_bytes,
                                          float* loss_out, void* stats_out, void* stream) {
    if (!logits || !target || !workspace || !loss_out || !stats_out) { msam_set_error("msam_semantic_loss_forward: null pointer"); return 1; }
    if (!sl_shape_ok(B, C, HW)) {
        static char msg[160];
        snprintf(msg, sizeof msg, "msam_semantic_loss_forward: %s", SL_SHAPE);
        msam_set_error(msg);
        return 1;
    }
    if (!sl_weights_ok(dice_weight, ce_weight, apply_softmax, eps)) {
        static char msg[256];
        snprintf(msg, sizeof msg, "msam_semantic_loss_forward: %s", SL_WEIGHTS);
        msam_set_error(msg);
        return 1;
    }
    if ((uintptr_t)workspace % 8 != 0 || (uintptr_t)stats_out % 8 != 0 || workspace_bytes < msam_semantic_loss_workspace_bytes(B, C, HW)) {
        msam_set_error("msam_semantic_loss_forward: workspace and stats_out must be 8-byte aligned, the workspace as large as "
                       "msam_semantic_loss_workspace_bytes says");
        return 1;
    }
    const long total = (long)B * HW;
    const unsigned nwg = (unsigned)((total + SL_PIX - 1) / SL_PIX);
    double* partD = (double*)workspace;
    int* partI = (int*)(partD + (size_t)nwg * (2 * C + 1));
    double* statsD = (double*)stats_out;
    long long* statsI = (long long*)(statsD + 2 * C + 3);
    hipStream_t s = (hipStream_t)stream;
    if (sl_vec(HW, logits, target, logits))
        sl_launch_sums<4>(nwg, s, logits, target, (int)C, (int)HW, total, (int)apply_softmax, partD, partI);
    else
        sl_launch_sums<1>(nwg, s, logits, target, (int)C, (int)HW, total, (int)apply_softmax, partD, partI);
    hipLaunchKernelGGL(sl_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)partD, (const int*)partI, (int)nwg, (int)C, dice_weight,
                       ce_weight, (int)apply_softmax, eps, loss_out, statsD, statsI);
    return msam_check_launch("msam_semantic_loss_forward");
}

extern "C" int msam_semantic_loss_backward(const float* logits, const int32_t* target, int32_t B, int32_t C, int32_t HW, float dice_weight,
                                           float ce_weight, int32_t apply_softmax, double eps, const void* stats, const float* grad_out_ptr,
                                           float* dlogits, void* stream) {
    if (!logits || !target || !stats || !grad_out_ptr || !dlogits) { msam_set_error("msam_semantic_loss_backward: null pointer"); return 1; }
    if (!sl_shape_ok(B, C, HW)) {
        static char msg[160];
        snprintf(msg, sizeof msg, "msam_semantic_loss_backward: %s", SL_SHAPE);
        msam_set_error(msg);
        return 1;
    }
    if (!sl_weights_ok(dice_weight, ce_weight, apply_softmax, eps)) {
        static char msg[256];
        snprintf(msg, sizeof msg, "msam_semantic_loss_backward: %s", SL_WEIGHTS);
        msam_set_error(msg);
        return 1;
    }
    if ((uintptr_t)stats % 8 != 0 || (uintptr_t)grad_out_ptr % 4 != 0) {
        msam_set_error("msam_semantic_loss_backward: stats must be 8-byte aligned, grad_out_ptr 4-byte aligned");
        return 1;
    }
    const long total = (long)B * HW;
    const unsigned nwg = (unsigned)((total + SL_PIX - 1) / SL_PIX);
    const double* statsD = (const double*)stats;
    const long long* statsI = (const long long*)(statsD + 2 * C + 3);
    hipStream_t s = (hipStream_t)stream;
    if (sl_vec(HW, logits, target, dlogits))
        sl_launch_backward<4>(nwg, s, logits, target, (int)C, (int)HW, total, dice_weight, ce_weight, (int)apply_softmax, eps, statsD, statsI,
                              grad_out_ptr, dlogits);
    else
        sl_launch_backward<1>(nwg, s, logits, target, (int)C, (int)HW, total, dice_weight, ce_weight, (int)apply_softmax, eps, statsD, statsI,
                              grad_out_ptr, dlogits);
    return msam_check_launch("msam_semantic_loss_backward");
}
