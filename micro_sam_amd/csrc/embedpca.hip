// Device side of micro_sam_amd.visualization: the PCA projection of image embeddings (reference micro_sam/visualization.py compute_pca,
// i.e. elf.segmentation.embeddings.embedding_pca on sklearn's PCA), for a batch of U units per call.  A unit is one embedding in its own
// channel-major layout: float32 [C, N], N = H * W positions, C <= 256 channels; no transposed copy is made.
//
//   moments : two passes.  pca_mean_kernel sums every channel in fp64 (one workgroup per channel: per-thread strided sums, a fixed LDS tree)
//             and stores the mean rounded to fp32.  pca_gram_kernel forms the Gram matrix of the CENTRED data x - mean on the f32-input MFMA
//             (v_mfma_f32_32x32x2_f32, exact fp32 products and an fp32 fmaf chain): a workgroup owns one 32 x 32 tile of the upper triangle
//             and one split of the positions; it stages 32 + 32 centred channel rows of 256 positions in LDS (global loads along N), each of its
//             four waves multiplies 64 positions of the chunk (32 MFMAs, fp32) and adds the result to fp64 registers, chunk after chunk.  The
//             four waves and then the splits are added in index order in fp64 (pca_gram_finish_kernel, which also mirrors the tile).  The
//             number of splits depends on N alone, so a unit's result does not depend on the batch it is part of.
//   project : out[u, j, n] = sum_c comp[u, j, c] (x[u, c, n] - mean[u, c]), one lane per position, c ascending, one fmaf per term;
//             pca_minmax_kernel then reduces the k * N values of a unit to their minimum and maximum (exact, so order-free).
//   to_rgb  : (255 (x - min)) / ptp in fp32 in that order, truncated to uint8, HWC; zeros where ptp == 0.
// No floating-point atomics anywhere; every sum has one fixed order, so two calls agree bit for bit.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

#if defined(__HIPCC__)
typedef float pca_f32x16_t __attribute__((ext_vector_type(16)));
#else
typedef f32x16_t pca_f32x16_t;                                          // (host compilation of the tests: the emulation's type)
#endif

constexpr int PCA_P = 256;                                              // positions per staged chunk: 64 per wave
constexpr int PCA_LD = PCA_P + 4;                                       // LDS row stride in floats: 16-byte aligned rows, 4 banks apart
constexpr int PCA_MAX_SPLITS = 16;

// splits of the positions of one unit and chunks per split: a function of N alone
inline void pca_splits(int N, int* splits, int* chunks_per_split) {
    const int nchunks = (N + PCA_P - 1) / PCA_P;
    int s = nchunks / 2;
    s = s < 1 ? 1 : (s > PCA_MAX_SPLITS ? PCA_MAX_SPLITS : s);
    const int cps = (nchunks + s - 1) / s;
    *chunks_per_split = cps;
    *splits = (nchunks + cps - 1) / cps;
}

// x [U, C, N]; grid (C, U): mean[u, c] = fp32(sum_n x / N), the sum in fp64
__global__ __launch_bounds__(256) void pca_mean_kernel(const float* __restrict__ x, int C, int N, float* __restrict__ mean) {
    __shared__ double red[256];
    const int tid = threadIdx.x, c = blockIdx.x, u = blockIdx.y;
    const float* __restrict__ p = x + ((size_t)u * C + c) * (size_t)N;
    double s = 0.0;
    for (int n = tid; n < N; n += 256) s += (double)p[n];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) mean[(size_t)u * C + c] = (float)(red[0] / (double)N);
}

// grid (pairs * splits, U).  partial [U, splits, pairs, 16, 64] fp64: accumulator register r of lane l, i.e. the tile element
// (row = (r & 3) + 8 (r >> 2) + 4 (l >> 5), col = l & 31)
__global__ __launch_bounds__(256) void pca_gram_kernel(const float* __restrict__ x, const float* __restrict__ mean, int C, int N, int tiles,
                                                        int pairs, int splits, int chunks_per_split, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float smem[2 * 32 * PCA_LD];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 31, lh = l >> 5;
    const int u = blockIdx.y;
    const int pair = blockIdx.x % pairs, split = blockIdx.x / pairs;
    int ti = 0, tj = pair;
    while (tj >= tiles - ti) { tj -= tiles - ti; ++ti; }
    tj += ti;
    const bool diag = ti == tj;
    float* As = smem;                                                   // (no __restrict__: on a diagonal tile B is A)
    float* Bs = diag ? smem : smem + 32 * PCA_LD;
    const float* __restrict__ xu = x + (size_t)u * C * (size_t)N;
    const float* __restrict__ mu = mean + (size_t)u * C;
    const int chunk0 = split * chunks_per_split;

    double dacc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) dacc[r] = 0.0;

    for (int ch = 0; ch < chunks_per_split; ++ch) {
        const long n = ((long)(chunk0 + ch)) * PCA_P + tid;             // the position this thread stages
        if ((long)(chunk0 + ch) * PCA_P >= N) break;                    // (uniform: the last split may be short)
        const bool inside = n < N;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
            const int ca = ti * 32 + r;
            float va = 0.f;
            if (inside && ca < C) va = __fsub_rn(xu[(size_t)ca * N + n], mu[ca]);
            As[r * PCA_LD + tid] = va;
            if (!diag) {
                const int cb = tj * 32 + r;
                float vb = 0.f;
                if (inside && cb < C) vb = __fsub_rn(xu[(size_t)cb * N + n], mu[cb]);
                Bs[r * PCA_LD + tid] = vb;
            }
        }
        __syncthreads();
        // lane (li, lh) of wave w: row li, positions w * 64 + lh * 32 .. + 31 of the chunk; MFMA m contracts positions m and 32 + m
        pca_f32x16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* ap = As + li * PCA_LD + w * 64 + lh * 32;
        const float* bp = Bs + li * PCA_LD + w * 64 + lh * 32;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(ap + 4 * q);
            const float4 b = *reinterpret_cast<const float4*>(bp + 4 * q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[r] += (double)acc[r];
        __syncthreads();                                                // the tiles are free for the next chunk (and for the reduction)
    }
    // the four waves in index order
    double* red = reinterpret_cast<double*>(smem);        // [4][16][64] doubles = 32 KiB of the 65 KiB
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * 16 + r) * 64 + l] = dacc[r];
    __syncthreads();
    double* __restrict__ dst = partial + (((size_t)u * splits + split) * pairs + pair) * 1024;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        dst[e] = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e];
    }
}

// grid (pairs, U): the splits in index order; the tile and its mirror image go to gram [U, C, C]
__global__ __launch_bounds__(256) void pca_gram_finish_kernel(const double* __restrict__ partial, int C, int tiles, int pairs, int splits,
                                                               double* __restrict__ gram) {
    const int tid = threadIdx.x, pair = blockIdx.x, u = blockIdx.y;
    int ti = 0, tj = pair;
    while (tj >= tiles - ti) { tj -= tiles - ti; ++ti; }
    tj += ti;
    double* __restrict__ g = gram + (size_t)u * C * C;
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q, r = e >> 6, l = e & 63;
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31;
        double s = 0.0;
        for (int sp = 0; sp < splits; ++sp) s += partial[(((size_t)u * splits + sp) * pairs + pair) * 1024 + e];
        const int i = ti * 32 + row, j = tj * 32 + col;
        if (i < C && j < C) {
            g[(size_t)i * C + j] = s;
            if (ti != tj) g[(size_t)j * C + i] = s;
        }
    }
}

// grid (ceil(N / 64), U), one wave per workgroup (a 64 x 64 unit makes 64 workgroups, not 16); comp [U, K, C], mean [U, C] -> out [U, K, N].
// KT: the compiled number of components (rows K..KT-1 are zeros)
template <int KT>
__global__ __launch_bounds__(64) void pca_project_kernel(const float* __restrict__ x, const float* __restrict__ comp,
                                                           const float* __restrict__ mean, int C, int N, int K, float* __restrict__ out) {
    __shared__ float cs[KT * 256];
    __shared__ float ms[256];
    const int tid = threadIdx.x, u = blockIdx.y;
    for (int i = tid; i < KT * 256; i += 64) {
        const int j = i >> 8, c = i & 255;
        cs[i] = (j < K && c < C) ? comp[((size_t)u * K + j) * C + c] : 0.f;
    }
    for (int c = tid; c < 256; c += 64) ms[c] = c < C ? mean[(size_t)u * C + c] : 0.f;
    __syncthreads();
    const long n = (long)blockIdx.x * 64 + tid;
    if (n >= N) return;
    const float* __restrict__ p = x + (size_t)u * C * (size_t)N + n;
    float acc[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) acc[j] = 0.f;
#pragma unroll 16
    for (int c = 0; c < C; ++c) {                                       // (16 independent loads in flight per lane)
        const float xc = __fsub_rn(p[(size_t)c * N], ms[c]);
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[j] = __fmaf_rn(cs[j * 256 + c], xc, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j < K) out[((size_t)u * K + j) * N + n] = acc[j];
}

// grid (U): minimum and maximum of the len values of unit u -> minmax [U, 2]
__global__ __launch_bounds__(256) void pca_minmax_kernel(const float* __restrict__ v, long len, float* __restrict__ minmax) {
    __shared__ float lo[256];
    __shared__ float hi[256];
    const int tid = threadIdx.x, u = blockIdx.x;
    const float* __restrict__ p = v + (size_t)u * len;
    float a = p[0], b = p[0];
    for (long i = tid; i < len; i += 256) { a = fminf(a, p[i]); b = fmaxf(b, p[i]); }
    lo[tid] = a; hi[tid] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { lo[tid] = fminf(lo[tid], lo[tid + o]); hi[tid] = fmaxf(hi[tid], hi[tid + o]); }
        __syncthreads();
    }
    if (tid == 0) { minmax[2 * u] = lo[0]; minmax[2 * u + 1] = hi[0]; }
}

// grid (ceil(N / 256), U); proj [U, 3, N] -> rgb [U, N, 3]
__global__ __launch_bounds__(256) void pca_to_rgb_kernel(const float* __restrict__ proj, const float* __restrict__ minmax, int N,
                                                          uint8_t* __restrict__ rgb) {
    const int u = blockIdx.y;
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float mn = minmax[2 * u], ptp = __fsub_rn(minmax[2 * u + 1], mn);
    for (int j = 0; j < 3; ++j) {
        int q = 0;
        if (ptp > 0.f) {
            const float t = __fdiv_rn(__fmul_rn(255.f, __fsub_rn(proj[((size_t)u * 3 + j) * N + n], mn)), ptp);
            q = (int)t;
            q = q < 0 ? 0 : (q > 255 ? 255 : q);
        }
        rgb[((size_t)u * N + n) * 3 + j] = (uint8_t)q;
    }
}

bool pca_shape_ok(int32_t U, int32_t C, int32_t N) {
    return U >= 1 && U <= MSAM_PCA_MAX_UNITS && C >= 1 && C <= MSAM_PCA_MAX_CHANNELS && N >= 1 && (int64_t)C * N < (1ll << 31);
}

}  // namespace

extern "C" int64_t msam_pca_moments_workspace_bytes(int32_t U, int32_t C, int32_t N) {
    if (!pca_shape_ok(U, C, N)) return 0;
    int splits, cps;
    pca_splits(N, &splits, &cps);
    const int tiles = (C + 31) / 32, pairs = tiles * (tiles + 1) / 2;
    return (int64_t)U * splits * pairs * 1024 * 8;
}

extern "C" int msam_pca_moments(const float* x, int32_t U, int32_t C, int32_t N, float* mean, double* gram, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    if (!x || !mean || !gram || !workspace) { msam_set_error("msam_pca_moments: null pointer"); return 1; }
    if (!pca_shape_ok(U, C, N)) {
        msam_set_error("msam_pca_moments: 1 <= U <= 65535 units of 1 <= C <= 256 channels and N >= 1 positions with C * N < 2^31");
        return 1;
    }
    if ((uintptr_t)workspace % 8 != 0 || workspace_bytes < msam_pca_moments_workspace_bytes(U, C, N)) {
        msam_set_error("msam_pca_moments: the workspace must be 8-byte aligned and as large as msam_pca_moments_workspace_bytes says");
        return 1;
    }
    int splits, cps;
    pca_splits(N, &splits, &cps);
    const int tiles = (C + 31) / 32, pairs = tiles * (tiles + 1) / 2;
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(pca_mean_kernel, dim3((unsigned)C, (unsigned)U), dim3(256), 0, s, x, (int)C, (int)N, mean);
    hipLaunchKernelGGL(pca_gram_kernel, dim3((unsigned)(pairs * splits), (unsigned)U), dim3(256), 0, s, x, (const float*)mean, (int)C, (int)N,
                       tiles, pairs, splits, cps, partial);
    hipLaunchKernelGGL(pca_gram_finish_kernel, dim3((unsigned)pairs, (unsigned)U), dim3(256), 0, s, (const double*)partial, (int)C, tiles, pairs,
                       splits, gram);
    return msam_check_launch("msam_pca_moments");
}

extern "C" int msam_pca_project(const float* x, const float* components, const float* mean, int32_t U, int32_t C, int32_t N, int32_t K,
                                float* out, float* minmax, void* stream) {
    if (!x || !components || !mean || !out || !minmax) { msam_set_error("msam_pca_project: null pointer"); return 1; }
    if (!pca_shape_ok(U, C, N) || K < 1 || K > MSAM_PCA_MAX_COMPONENTS) {
        msam_set_error("msam_pca_project: 1 <= U <= 65535 units of 1 <= C <= 256 channels and N >= 1 positions with C * N < 2^31, "
                       "1 <= K <= 8 components");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)U);
    if (K <= 3)
        hipLaunchKernelGGL((pca_project_kernel<3>), grid, dim3(64), 0, s, x, components, mean, (int)C, (int)N, (int)K, out);
    else
        hipLaunchKernelGGL((pca_project_kernel<8>), grid, dim3(64), 0, s, x, components, mean, (int)C, (int)N, (int)K, out);
    hipLaunchKernelGGL(pca_minmax_kernel, dim3((unsigned)U), dim3(256), 0, s, (const float*)out, (long)K * N, minmax);
    return msam_check_launch("msam_pca_project");
}

extern "C" int msam_pca_to_rgb(const float* proj, const float* minmax, int32_t U, int32_t N, uint8_t* rgb, void* stream) {
    if (!proj || !minmax || !rgb) { msam_set_error("msam_pca_to_rgb: null pointer"); return 1; }
    if (U < 1 || U > MSAM_PCA_MAX_UNITS || N < 1 || (int64_t)3 * N >= (1ll << 31)) {
        msam_set_error("msam_pca_to_rgb: 1 <= U <= 65535 units of 1 <= N < 2^31 / 3 positions");
        return 1;
    }
    hipLaunchKernelGGL(pca_to_rgb_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)U), dim3(256), 0, (hipStream_t)stream, proj, minmax,
                       (int)N, rgb);
    return msam_check_launch("msam_pca_to_rgb");
}
