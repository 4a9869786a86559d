// Device side of micro_sam_amd.evaluation: B predicted label images scored against ground truth in one call (the contingency table,
// object counts and IoU edges behind elf.evaluation.matching / mean_segmentation_accuracy, which the reference's
// micro_sam/evaluation/ calls per image on the host).  Integer work, bound by memory and atomics; no GEMM shape anywhere.
//
//   count : one open-addressing table per batch item, key = pred id << 32 | gt id, background pairs included.  A thread reads 16
//           consecutive pixels of both images (four 16-byte loads each), pre-sums runs of equal pairs, a workgroup aggregates its pairs
//           in an LDS table and flushes one global update per distinct pair (the aggregation of segment.hip's overlap_count_kernel).
//   areas : over the TABLE, not the pixels: every entry adds its count to the row sum of its pred id and the column sum of its gt id
//           (two id tables per batch item); the first entry of a non-zero id counts the object.
//   score : over the table: IoU of every pair of non-zero ids in fp64 - the IEEE division numpy performs in elf's
//           intersection_over_union -, one counter per threshold (aggregated per workgroup in LDS), and the compacted edge list.
// Every sum is an integer, so the results do not depend on the order of the atomics; only the ORDER of the edge list does.
#include "common.h"
#include "../../include/msam_hip.h"

void msam_set_error(const char* msg);
int msam_check_launch(const char* what);

namespace {

typedef unsigned long long u64;
constexpr u64 MT_EMPTY = ~0ull;
constexpr int MT_NOID = -1;
constexpr int MT_HDR = MSAM_MATCH_HEADER, MT_ITEM = MSAM_MATCH_ITEM, MT_EDGE = MSAM_MATCH_EDGE;
constexpr unsigned MT_MAX_PROBE = 4096;

struct MatchThresholds { double t[MSAM_MATCH_MAX_THRESHOLDS]; double tmin; int n; };

__device__ __forceinline__ unsigned mt_hash(u64 k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; return (unsigned)k; }

__device__ __forceinline__ void mt_pair_add(u64* __restrict__ keys, int* __restrict__ counts, unsigned mask, u64 key, int c,
                                            int* __restrict__ overflow) {
    unsigned h = mt_hash(key) & mask;
    for (unsigned probe = 0; probe <= mask && probe < MT_MAX_PROBE; ++probe, h = (h + 1) & mask) {
        const u64 prev = atomicCAS(&keys[h], MT_EMPTY, key);
        if (prev == MT_EMPTY || prev == key) { atomicAdd(&counts[h], c); return; }
    }
    atomicExch(overflow, 1);
}

// id table: area[id] += c; the entry that creates a non-zero id counts the object
__device__ __forceinline__ void mt_id_add(int* __restrict__ ids, int* __restrict__ area, unsigned mask, int id, int c,
                                          int* __restrict__ n_objects, int* __restrict__ overflow) {
    unsigned h = mt_hash((u64)(uint32_t)id) & mask;
    for (unsigned probe = 0; probe <= mask && probe < MT_MAX_PROBE; ++probe, h = (h + 1) & mask) {
        const int prev = atomicCAS(&ids[h], MT_NOID, id);
        if (prev == MT_NOID || prev == id) {
            atomicAdd(&area[h], c);
            if (prev == MT_NOID && id != 0) atomicAdd(n_objects, 1);
            return;
        }
    }
    atomicExch(overflow, 1);
}

__device__ __forceinline__ int mt_id_area(const int* __restrict__ ids, const int* __restrict__ area, unsigned mask, int id) {
    unsigned h = mt_hash((u64)(uint32_t)id) & mask;
    for (unsigned probe = 0; probe <= mask && probe < MT_MAX_PROBE; ++probe, h = (h + 1) & mask) {
        const int k = ids[h];
        if (k == id) return area[h];
        if (k == MT_NOID) break;
    }
    return -1;                                                         // (only after an overflow)
}

// pred [B, npx], gt [G, npx] (gt_stride = 0: one image for every batch item); blockIdx.y = batch item.  WIDE: npx % 4 == 0 and both
// bases 16-byte aligned, so every full span of 16 pixels is four aligned 16-byte loads per image.
template <bool WIDE>
__global__ __launch_bounds__(256) void match_count_kernel(const int* __restrict__ pred, const int* __restrict__ gt, long gt_stride, int npx,
                                                          u64* __restrict__ keys, int* __restrict__ counts, unsigned cap,
                                                          int* __restrict__ result) {
    constexpr int TAB = 1024, PER = 16;
    __shared__ u64 lk[TAB];
    __shared__ int lv[TAB];
    for (int i = threadIdx.x; i < TAB; i += 256) { lk[i] = MT_EMPTY; lv[i] = 0; }
    __syncthreads();
    const int b = blockIdx.y;
    u64* __restrict__ bkeys = keys + (size_t)b * cap;
    int* __restrict__ bcounts = counts + (size_t)b * cap;
    int* __restrict__ overflow = result + MT_HDR + b * MT_ITEM + 3;
    const unsigned mask = cap - 1;
    auto flush = [&](u64 key, int c) {
        if (c == 0) return;
        unsigned h = mt_hash(key) & (TAB - 1);
        for (int probe = 0; probe < 24; ++probe, h = (h + 1) & (TAB - 1)) {
            const u64 prev = atomicCAS(&lk[h], MT_EMPTY, key);
            if (prev == MT_EMPTY || prev == key) { atomicAdd(&lv[h], c); return; }
        }
        mt_pair_add(bkeys, bcounts, mask, key, c, overflow);           // LDS table crowded
    };
    const long base = ((long)blockIdx.x * 256 + threadIdx.x) * PER;
    const int n = base >= npx ? 0 : (npx - base < PER ? (int)(npx - base) : PER);
    const int* __restrict__ pp = pred + (size_t)b * npx + base;
    const int* __restrict__ gp = gt + (size_t)b * gt_stride + base;
    int pv[PER], gv[PER];
    if (WIDE && n == PER) {
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const uint4 a = *reinterpret_cast<const uint4*>(pp + 4 * q);
            const uint4 c = *reinterpret_cast<const uint4*>(gp + 4 * q);
            pv[4 * q] = (int)a.x; pv[4 * q + 1] = (int)a.y; pv[4 * q + 2] = (int)a.z; pv[4 * q + 3] = (int)a.w;
            gv[4 * q] = (int)c.x; gv[4 * q + 1] = (int)c.y; gv[4 * q + 2] = (int)c.z; gv[4 * q + 3] = (int)c.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) { pv[k] = k < n ? pp[k] : 0; gv[k] = k < n ? gp[k] : 0; }
    }
    u64 cur = MT_EMPTY; int cnt = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (k < n) {
            const u64 key = ((u64)(uint32_t)pv[k] << 32) | (u64)(uint32_t)gv[k];
            if (key == cur) ++cnt;
            else { flush(cur, cnt); cur = key; cnt = 1; }
        }
    }
    flush(cur, cnt);
    __syncthreads();
    for (int i = threadIdx.x; i < TAB; i += 256)
        if (lk[i] != MT_EMPTY) mt_pair_add(bkeys, bcounts, mask, lk[i], lv[i], overflow);
}

// one thread per slot of the B pair tables (cap is a multiple of 256: a workgroup stays inside one batch item)
__global__ __launch_bounds__(256) void match_area_kernel(const u64* __restrict__ keys, const int* __restrict__ counts, unsigned cap,
                                                         int* __restrict__ pid, int* __restrict__ parea, int* __restrict__ gid,
                                                         int* __restrict__ garea, int* __restrict__ result) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int b = (int)(i / cap);
    const u64 key = keys[i];
    if (key == MT_EMPTY) return;
    int* __restrict__ item = result + MT_HDR + b * MT_ITEM;
    const size_t o = (size_t)b * cap;
    const int c = counts[i];
    mt_id_add(pid + o, parea + o, cap - 1, (int)(key >> 32), c, item + 0, item + 3);
    mt_id_add(gid + o, garea + o, cap - 1, (int)(uint32_t)key, c, item + 1, item + 3);
}

__global__ __launch_bounds__(256) void match_score_kernel(const u64* __restrict__ keys, const int* __restrict__ counts, unsigned cap,
                                                          const int* __restrict__ pid, const int* __restrict__ parea,
                                                          const int* __restrict__ gid, const int* __restrict__ garea,
                                                          MatchThresholds thr, int max_edges, int* __restrict__ result,
                                                          int* __restrict__ edges) {
    __shared__ int tc[MSAM_MATCH_MAX_THRESHOLDS];
    if (threadIdx.x < MSAM_MATCH_MAX_THRESHOLDS) tc[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int b = (int)(i / cap);
    const size_t o = (size_t)b * cap;
    const u64 key = keys[i];
    const int p = (int)(key >> 32), g = (int)(uint32_t)key;
    if (key != MT_EMPTY && p != 0 && g != 0) {
        const int c = counts[i];
        const int ap = mt_id_area(pid + o, parea + o, cap - 1, p), ag = mt_id_area(gid + o, garea + o, cap - 1, g);
        if (ap >= 0 && ag >= 0) {
            // int32 areas of an image of < 2^31 pixels: the union fits a long, and a double holds it exactly
            const double score = (double)c / fmax((double)((long)ap + (long)ag - (long)c), 1e-7);
            for (int t = 0; t < thr.n; ++t)
                if (score >= thr.t[t]) atomicAdd(&tc[t], 1);
            if (score >= thr.tmin) {
                const int slot = atomicAdd(&result[0], 1);
                if (slot < max_edges) {
                    int* __restrict__ e = edges + (size_t)slot * MT_EDGE;
                    e[0] = b; e[1] = p; e[2] = g; e[3] = c; e[4] = ap; e[5] = ag;
                } else atomicExch(&result[1], 1);                      // edge list too small
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < thr.n && tc[threadIdx.x] != 0) atomicAdd(&result[MT_HDR + b * MT_ITEM + 4 + threadIdx.x], tc[threadIdx.x]);
}

}  // namespace

extern "C" int64_t msam_label_matching_workspace_bytes(int32_t B, int32_t capacity) {
    if (B < 1 || B > MSAM_MATCH_MAX_BATCH || capacity < 1024 || (capacity & (capacity - 1)) || (int64_t)B * capacity > (1ll << 31)) return 0;
    return (int64_t)B * capacity * 28;                                 // keys 8, counts 4, two id tables of (id 4, area 4)
}

extern "C" int msam_label_matching(const int32_t* pred, const int32_t* gt, int32_t B, int32_t G, int32_t H, int32_t W,
                                   const double* thresholds, int32_t T, void* workspace, int64_t workspace_bytes, int32_t capacity,
                                   int32_t* result, int32_t max_edges, void* stream) {
    if (!pred || !gt || !thresholds || !workspace || !result) { msam_set_error("msam_label_matching: null pointer"); return 1; }
    if (B < 1 || B > MSAM_MATCH_MAX_BATCH || (G != 1 && G != B)) {
        msam_set_error("msam_label_matching: 1 <= B <= 65535 predictions against G == B or G == 1 ground-truth images");
        return 1;
    }
    if (T < 1 || T > MSAM_MATCH_MAX_THRESHOLDS) { msam_set_error("msam_label_matching: 1 <= T <= 16 thresholds"); return 1; }
    if (H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) { msam_set_error("msam_label_matching: H, W > 0 and H * W < 2^31"); return 1; }
    if (capacity < 1024 || (capacity & (capacity - 1)) || (int64_t)B * capacity > (1ll << 31) || max_edges < 1 ||
        workspace_bytes < msam_label_matching_workspace_bytes(B, capacity)) {
        msam_set_error("msam_label_matching: capacity must be a power of two >= 1024 with B * capacity <= 2^31, max_edges >= 1 and "
                       "the workspace as large as msam_label_matching_workspace_bytes says");
        return 1;
    }
    MatchThresholds thr;
    thr.n = T;
    thr.tmin = thresholds[0];
    for (int t = 0; t < MSAM_MATCH_MAX_THRESHOLDS; ++t) {
        thr.t[t] = t < T ? thresholds[t] : 0.0;
        if (t < T && !(thresholds[t] == thresholds[t])) { msam_set_error("msam_label_matching: a threshold is NaN"); return 1; }
        if (t < T && thresholds[t] < thr.tmin) thr.tmin = thresholds[t];
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t slots = (size_t)B * capacity;
    // workspace: [keys u64 | pred ids | gt ids] start as all-ones (empty), [counts | pred areas | gt areas] as zeros
    u64* keys = (u64*)workspace;
    int* pid = (int*)(keys + slots);
    int* gid = pid + slots;
    int* counts = gid + slots;
    int* parea = counts + slots;
    int* garea = parea + slots;
    if (hipMemsetAsync(keys, 0xff, slots * 16, s) != hipSuccess || hipMemsetAsync(counts, 0, slots * 12, s) != hipSuccess ||
        hipMemsetAsync(result, 0, ((size_t)MT_HDR + (size_t)B * MT_ITEM) * 4, s) != hipSuccess) {
        msam_set_error("msam_label_matching: memset failed");
        return 2;
    }
    const int npx = H * W;
    const unsigned gx = (unsigned)(((long)npx + 4095) / 4096);
    const long gt_stride = G == 1 ? 0 : (long)npx;
    const bool wide = npx % 4 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)gt % 16 == 0;
    if (wide)
        hipLaunchKernelGGL((match_count_kernel<true>), dim3(gx, (unsigned)B), dim3(256), 0, s, pred, gt, gt_stride, npx, keys, counts,
                           (unsigned)capacity, result);
    else
        hipLaunchKernelGGL((match_count_kernel<false>), dim3(gx, (unsigned)B), dim3(256), 0, s, pred, gt, gt_stride, npx, keys, counts,
                           (unsigned)capacity, result);
    const unsigned tb = (unsigned)(slots / 256);
    hipLaunchKernelGGL(match_area_kernel, dim3(tb), dim3(256), 0, s, (const u64*)keys, (const int*)counts, (unsigned)capacity, pid, parea,
                       gid, garea, result);
    hipLaunchKernelGGL(match_score_kernel, dim3(tb), dim3(256), 0, s, (const u64*)keys, (const int*)counts, (unsigned)capacity,
                       (const int*)pid, (const int*)parea, (const int*)gid, (const int*)garea, thr, max_edges, result,
                       result + MT_HDR + (size_t)B * MT_ITEM);
    return msam_check_launch("msam_label_matching");
}
