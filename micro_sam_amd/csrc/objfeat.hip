// Device side of micro_sam.object_classification (compute_object_features / project_prediction_to_segmentation): per-object means
// of the SAM image embedding resampled onto the label grid, the restatement of skimage's resize + regionprops_table
// (micro_sam/object_classification.py:20-57).  A UNIT is one embedding plus the part of the label image it covers (the 2-D image,
// one tile's outer block, one slice, or one tile of one slice).  Per unit the host gives the resize tables (double precision,
// object_classification.py): the nearest-neighbour source row / column of every resized label pixel in the zero-padded square label
// image (a source index past the unit's extent is padding: label 0) and the two bilinear taps + weight per axis of the embedding.
//
//   gather     : one thread per resized pixel: label -> object index (binary search in the sorted ids, -1 = background), integer
//                area atomics, sort key object * U + unit (background: INT64_MAX).  The caller sorts the keys (stable): every
//                object's pixels become contiguous, in (unit, raster) order.
//   accumulate : one wave per chunk of <= K consecutive sorted pixels of one object; lanes span the 256 channels, 4 each (float4
//                loads from the unit's CHANNEL-LAST embedding: every tap is 1 KiB contiguous); the bilinear value in fp32, the sum in
//                fp64; one fp64 partial row per chunk.  Bound by the L2 / MALL reads of the taps (4 x 1 KiB per pixel).
//   finish     : per object, the chunk partials added in chunk order (fp64) to the running sums of earlier batches; on the last
//                batch the (area, means) row is written as fp32 or fp64.  No floating-point atomics anywhere: results are
//                bit-identical from call to call.
//   project    : per label pixel, the index of its id in the sorted id table (-1 when absent), for project_prediction_to_segmentation.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

#define OF_INT64_MAX 0x7fffffffffffffffLL

// unit descriptor fields (int64 [U, MSAM_OBJFEAT_DESC]; include/msam_hip.h)
enum { D_LAB_OFF = 0, D_LAB_LD, D_LAB_H, D_LAB_W, D_EMB_OFF, D_EMB_W, D_RH, D_RW, D_ITAB, D_FTAB, D_PIX, D_EMB_H };

MSAM_DEVINL long long of_find(const long long* __restrict__ ids, int n, long long v) {     // index of v in ids[0, n), -1 if absent
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && ids[lo] == v) ? lo : -1;
}

__global__ __launch_bounds__(256) void objfeat_gather_kernel(const long long* __restrict__ labels, const long long* __restrict__ desc,
                                                             const int* __restrict__ itab, const long long* __restrict__ ids, int n_ids,
                                                             int U, long long* __restrict__ keys, int* __restrict__ area) {
    const int u = blockIdx.y;
    const long long* d = desc + (long)u * MSAM_OBJFEAT_DESC;
    const int Rh = (int)d[D_RH], Rw = (int)d[D_RW];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Rh * Rw) return;
    const int oy = p / Rw, ox = p - oy * Rw;
    const int* t = itab + d[D_ITAB];                        // ly[Rh], y0[Rh], y1[Rh], lx[Rw], x0[Rw], x1[Rw]
    const int sy = t[oy], sx = t[3 * Rh + ox];
    long long v = 0;
    if (sy < d[D_LAB_H] && sx < d[D_LAB_W]) v = labels[d[D_LAB_OFF] + (long long)sy * d[D_LAB_LD] + sx];
    long long key = OF_INT64_MAX;
    if (v != 0) {
        const long long o = of_find(ids, n_ids, v);
        if (o >= 0) {
            key = o * U + u;
            atomicAdd(&area[o], 1);
        }
    }
    keys[d[D_PIX] + p] = key;
}

// one wave per chunk; chunk_start int32 [N + 1] (exclusive prefix of ceil(area / K)), pix_start int64 [N] (exclusive prefix of area)
__global__ __launch_bounds__(256) void objfeat_accumulate_kernel(const float* __restrict__ emb, const long long* __restrict__ desc,
                                                                 const int* __restrict__ itab, const float* __restrict__ ftab,
                                                                 const long long* __restrict__ sorted_keys, const long long* __restrict__ perm,
                                                                 const int* __restrict__ chunk_start, const long long* __restrict__ pix_start,
                                                                 const int* __restrict__ area, int n_ids, int U, int K,
                                                                 double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= chunk_start[n_ids]) return;
    int lo = 0, hi = n_ids;                                  // object: the last o with chunk_start[o] <= c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= c) lo = mid; else hi = mid;
    }
    const int o = lo;
    const long long i0 = pix_start[o] + (long long)(c - chunk_start[o]) * K;
    const long long end = pix_start[o] + area[o], i1 = i0 + K < end ? i0 + K : end;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (long long i = i0; i < i1; ++i) {
        const int u = (int)(sorted_keys[i] % U);
        const long long* d = desc + (long)u * MSAM_OBJFEAT_DESC;
        const int Rh = (int)d[D_RH], Rw = (int)d[D_RW];
        const int q = (int)(perm[i] - d[D_PIX]);
        const int oy = q / Rw, ox = q - oy * Rw;
        const int* t = itab + d[D_ITAB];
        const float* w = ftab + d[D_FTAB];                    // wy[Rh], wx[Rw]
        const int y0 = t[Rh + oy], y1 = t[2 * Rh + oy], x0 = t[3 * Rh + Rw + ox], x1 = t[3 * Rh + 2 * Rw + ox];
        const float wy = w[oy], wx = w[Rh + ox];
        const long long ew = d[D_EMB_W];
        const float* e = emb + d[D_EMB_OFF] + 4 * lane;
        const float4 v00 = *reinterpret_cast<const float4*>(e + (y0 * ew + x0) * 256);
        const float4 v01 = *reinterpret_cast<const float4*>(e + (y0 * ew + x1) * 256);
        const float4 v10 = *reinterpret_cast<const float4*>(e + (y1 * ew + x0) * 256);
        const float4 v11 = *reinterpret_cast<const float4*>(e + (y1 * ew + x1) * 256);
        const float ux = 1.f - wx, uy = 1.f - wy;
        a0 += (double)(uy * (ux * v00.x + wx * v01.x) + wy * (ux * v10.x + wx * v11.x));
        a1 += (double)(uy * (ux * v00.y + wx * v01.y) + wy * (ux * v10.y + wx * v11.y));
        a2 += (double)(uy * (ux * v00.z + wx * v01.z) + wy * (ux * v10.z + wx * v11.z));
        a3 += (double)(uy * (ux * v00.w + wx * v01.w) + wy * (ux * v10.w + wx * v11.w));
    }
    double* out = partial + (long)c * 256 + 4 * lane;
    out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
}

// one workgroup per object, one thread per channel
__global__ __launch_bounds__(256) void objfeat_finish_kernel(const double* __restrict__ partial, const int* __restrict__ chunk_start,
                                                             const int* __restrict__ area, double* __restrict__ sums,
                                                             long long* __restrict__ area_total, int out_f64, void* out) {
    const int o = blockIdx.x, ch = threadIdx.x;
    double s = 0.0;
    for (int c = chunk_start[o]; c < chunk_start[o + 1]; ++c) s += partial[(long)c * 256 + ch];
    const double total = sums[(long)o * 256 + ch] + s;
    sums[(long)o * 256 + ch] = total;
    const long long a = area_total[o] + area[o];
    __syncthreads();                                          // (every thread has read area_total[o] before it is updated)
    if (ch == 0) area_total[o] = a;
    if (!out) return;
    const double mean = a > 0 ? total / (double)a : 0.0;
    if (out_f64) {
        double* row = (double*)out + (long)o * 257;
        if (ch == 0) row[0] = (double)a;
        row[1 + ch] = mean;
    } else {
        float* row = (float*)out + (long)o * 257;
        if (ch == 0) row[0] = (float)a;
        row[1 + ch] = (float)mean;
    }
}

__global__ __launch_bounds__(256) void objfeat_project_kernel(const long long* __restrict__ labels, long long n,
                                                              const long long* __restrict__ ids, int n_ids, int* __restrict__ index) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    index[i] = (int)of_find(ids, n_ids, labels[i]);
}

}  // namespace

extern "C" int msam_objfeat_gather(const int64_t* labels, const int64_t* desc, int32_t U, int32_t max_pixels, const int32_t* itab,
                                   const int64_t* ids, int32_t n_ids, int64_t* keys, int32_t* area, void* stream) {
    if (!labels || !desc || !itab || !keys || !area || U <= 0 || U > 65535 || max_pixels <= 0 || n_ids <= 0 || !ids) {
        msam_set_error("msam_objfeat_gather: bad arguments");
        return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(area, 0, (size_t)n_ids * 4, s) != hipSuccess) { msam_set_error("msam_objfeat_gather: memset failed"); return 2; }
    hipLaunchKernelGGL(objfeat_gather_kernel, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)U), dim3(256), 0, s,
                       (const long long*)labels, (const long long*)desc, itab, (const long long*)ids, n_ids, U, (long long*)keys, area);
    return msam_check_launch("msam_objfeat_gather");
}

extern "C" int msam_objfeat_accumulate(const float* emb, const int64_t* desc, int32_t U, const int32_t* itab, const float* ftab,
                                       const int64_t* sorted_keys, const int64_t* perm, const int32_t* chunk_start, const int64_t* pix_start,
                                       const int32_t* area, int32_t n_ids, int32_t K, int32_t max_chunks, double* partial, void* stream) {
    if (!emb || !desc || !itab || !ftab || !sorted_keys || !perm || !chunk_start || !pix_start || !area || !partial || U <= 0 ||
        n_ids <= 0 || K <= 0 || max_chunks <= 0) {
        msam_set_error("msam_objfeat_accumulate: bad arguments");
        return 1;
    }
    hipLaunchKernelGGL(objfeat_accumulate_kernel, dim3((unsigned)((max_chunks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, emb,
                       (const long long*)desc, itab, ftab, (const long long*)sorted_keys, (const long long*)perm, chunk_start,
                       (const long long*)pix_start, area, n_ids, U, K, partial);
    return msam_check_launch("msam_objfeat_accumulate");
}

extern "C" int msam_objfeat_finish(const double* partial, const int32_t* chunk_start, const int32_t* area, int32_t n_ids, double* sums,
                                   int64_t* area_total, int32_t out_f64, void* out, void* stream) {
    if (!partial || !chunk_start || !area || !sums || !area_total || n_ids <= 0 || (out_f64 != 0 && out_f64 != 1)) {
        msam_set_error("msam_objfeat_finish: bad arguments");
        return 1;
    }
    hipLaunchKernelGGL(objfeat_finish_kernel, dim3((unsigned)n_ids), dim3(256), 0, (hipStream_t)stream, partial, chunk_start, area, sums,
                       (long long*)area_total, out_f64, out);
    return msam_check_launch("msam_objfeat_finish");
}

extern "C" int msam_objfeat_project(const int64_t* labels, int64_t n, const int64_t* ids, int32_t n_ids, int32_t* index, void* stream) {
    if (!labels || !index || n <= 0 || n_ids < 0 || (n_ids > 0 && !ids) || (n + 255) / 256 > 0x7fffffffLL) {
        msam_set_error("msam_objfeat_project: bad arguments");
        return 1;
    }
    hipLaunchKernelGGL(objfeat_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)labels, (long long)n, (const long long*)ids, n_ids, index);
    return msam_check_launch("msam_objfeat_project");
}
