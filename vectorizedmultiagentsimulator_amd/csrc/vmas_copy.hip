// vmas_copy.hip -- one launch for a list of device-to-device byte copies (graph mode's carried
// state, output clones and per-step backups; simulator/environment/_graph.py).
//
// torch._foreach_copy_ over the handful of large tensors a step hands on launched PyTorch's
// multi-tensor-apply kernel once per dtype and call site (4 launches per balance step, 75-171
// workgroups each, 40 us of GPU time for ~14 MB).  Here every span of a call -- whatever its
// dtype -- goes in ONE launch: blockIdx.y = span, blockIdx.x grid-strides over the span in 16-byte
// (or, for unaligned spans, 4- / 1-byte) units, 256 threads x 4 units per workgroup round.
// HBM-bound: 2 x bytes of traffic.
//
// Also k_masked_rows (vmas_masked_rows): per-row copies under a mask, the merge launch of
// Environment.reset_where's generic path (simulator/environment/_masked.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vmas_aux.hpp"
#include "vmas_mi355x.h"
#include "vmas_uniform.hpp"

namespace {

constexpr int kCopyThreads = 256, kCopyUnroll = 4, kMaxCopyBlocks = 1024;

struct CopyArgs {
    VmasCopySpan s[VMAS_COPY_MAX_SPANS];
    int n;
};
static_assert(sizeof(CopyArgs) <= 4096, "kernel argument block");

// blk / nblk: this workgroup's index among the span's nblk workgroups (grid-stride over them)
template <typename T>
__device__ __forceinline__ void copy_units(const T* __restrict__ src, T* __restrict__ dst, int64_t n, int blk, int nblk) {
    const int64_t step = (int64_t)nblk * kCopyThreads;
    int64_t i = (int64_t)blk * kCopyThreads + threadIdx.x;
    for (; i + (kCopyUnroll - 1) * step < n; i += kCopyUnroll * step) {
        T v[kCopyUnroll];
#pragma unroll
        for (int k = 0; k < kCopyUnroll; ++k) v[k] = src[i + k * step];  // independent loads in flight
#pragma unroll
        for (int k = 0; k < kCopyUnroll; ++k) dst[i + k * step] = v[k];
    }
    for (; i < n; i += step) dst[i] = src[i];
}

__device__ __forceinline__ void copy_span(const VmasCopySpan& s, int blk, int nblk) {
    if (s.nbytes == VMAS_COPY_STORE64) {  // a store span: the 8-byte value src at dst
        if (blk == 0 && threadIdx.x == 0) *reinterpret_cast<uint64_t*>(s.dst) = (uint64_t)(uintptr_t)s.src;
        return;
    }
    if (!s.src) {  // an increment span: dst[i] += 1.0f
        float* d = reinterpret_cast<float*>(s.dst);
        const int64_t n = s.nbytes / 4;
        for (int64_t i = (int64_t)blk * kCopyThreads + threadIdx.x; i < n; i += (int64_t)nblk * kCopyThreads)
            d[i] = d[i] + 1.0f;
        return;
    }
    const uintptr_t al = (uintptr_t)s.src | (uintptr_t)s.dst | (uintptr_t)s.nbytes;
    if ((al & 15) == 0)
        copy_units(reinterpret_cast<const uint4*>(s.src), reinterpret_cast<uint4*>(s.dst), s.nbytes / 16, blk, nblk);
    else if ((al & 3) == 0)
        copy_units(reinterpret_cast<const uint32_t*>(s.src), reinterpret_cast<uint32_t*>(s.dst), s.nbytes / 4, blk, nblk);
    else
        copy_units(reinterpret_cast<const uint8_t*>(s.src), reinterpret_cast<uint8_t*>(s.dst), s.nbytes, blk, nblk);
}

__global__ void __launch_bounds__(kCopyThreads) k_copy_spans(CopyArgs a) {
    copy_span(a.s[blockIdx.y], (int)blockIdx.x, (int)gridDim.x);
}

// The post-replay copies and the next step's random-action draw in ONE launch (vmas_copy_spans_draw).
// Packed grid: item y (span y < n_spans, else draw column y - n_spans) owns the 1-D workgroups
// [first[y], first[y + 1]) -- a copy span as many as its bytes need (<= 1024), a column exactly
// torch's gx_draw -- so no workgroup is launched only to leave (a 2-D grid of max(copy, draw) x
// items launched ~10 000 of them per step for ~1 000 that work; measured, rejected and removed
// with the non-temporal-store and units-per-thread variants, last held by commit 7ff9a7c).
constexpr int kMergedSpans = 96, kMergedCols = 16;
struct CopyDrawArgs {
    VmasCopySpan s[kMergedSpans];
    VmasUniformColumn c[kMergedCols];
    unsigned long long seed;
    long long numel, snap;
    const unsigned long long* off_dev;  // (non-null: the columns' offsets are relative to *off_dev)
    int n_spans, gx_draw, mode, n_items;
    int first[kMergedSpans + kMergedCols + 1];  // the items' first workgroups (n_items + 1)
};
static_assert(sizeof(CopyDrawArgs) <= 4096, "kernel argument block");

__global__ void __launch_bounds__(kCopyThreads) k_copy_draw(CopyDrawArgs a) {
    // the item owning this workgroup: the last y with first[y] <= blockIdx.x
    const int bx = (int)blockIdx.x;
    int lo = 0, hi = a.n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.first[mid] <= bx) lo = mid;
        else hi = mid - 1;
    }
    const int y = lo, blk = bx - a.first[y];
    if (y < a.n_spans) {
        copy_span(a.s[y], blk, a.first[y + 1] - a.first[y]);
        return;
    }
    VmasUniformColumn col = a.c[y - a.n_spans];
    if (a.off_dev) col.offset += *a.off_dev;  // (the generator offset a device launch left: see the ABI)
    vmas_uniform::draw_column(col, a.seed, a.numel, a.snap, a.mode, a.gx_draw, blk);
}

constexpr int kFillThreads = 256;

__global__ void __launch_bounds__(kFillThreads) k_fill_u32(uint32_t* __restrict__ dst, uint32_t value, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kFillThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kFillThreads)
        dst[i] = value;
}

// ---- masked rows (vmas_masked_rows; Environment.reset_where) ------------------------------------
// blockIdx.y = span; the span's batch x (row_bytes / unit) units are taken in order by consecutive
// threads (grid-stride): the units of a row, then the next row -- whole lines of a contiguous [B, k]
// tensor.  A row is copied src -> dst when (mask[row] != 0) == want; the others are not touched.
struct MaskedArgs {
    VmasMaskedSpan s[VMAS_MASKED_MAX_SPANS];
    const uint8_t* mask;
    long long batch;
    int want;
};
static_assert(sizeof(MaskedArgs) <= 4096, "kernel argument block");

__host__ __device__ __forceinline__ int masked_unit(const VmasMaskedSpan& s) {
    const uintptr_t al = (uintptr_t)s.src | (uintptr_t)s.dst | (uintptr_t)s.row_bytes | (uintptr_t)s.dst_stride |
                         (uintptr_t)s.src_stride;
    return (al & 15) == 0 ? 16 : (al & 7) == 0 ? 8 : (al & 3) == 0 ? 4 : 1;
}

template <typename T>
__device__ __forceinline__ void masked_units(const VmasMaskedSpan& s, const uint8_t* __restrict__ mask, long long batch,
                                             bool want) {
    const long long k = s.row_bytes / (long long)sizeof(T), n = batch * k;
    const long long step = (long long)gridDim.x * kCopyThreads;
    for (long long i = (long long)blockIdx.x * kCopyThreads + threadIdx.x; i < n; i += step) {
        const long long row = k == 1 ? i : i / k, c = k == 1 ? 0 : i - row * k;
        if ((mask[row] != 0) != want) continue;
        const T v = *reinterpret_cast<const T*>(static_cast<const char*>(s.src) + row * s.src_stride + c * (long long)sizeof(T));
        *reinterpret_cast<T*>(static_cast<char*>(s.dst) + row * s.dst_stride + c * (long long)sizeof(T)) = v;
    }
}

__global__ void __launch_bounds__(kCopyThreads) k_masked_rows(MaskedArgs a) {
    const VmasMaskedSpan s = a.s[blockIdx.y];
    switch (masked_unit(s)) {
        case 16: masked_units<uint4>(s, a.mask, a.batch, a.want != 0); break;
        case 8: masked_units<uint2>(s, a.mask, a.batch, a.want != 0); break;
        case 4: masked_units<uint32_t>(s, a.mask, a.batch, a.want != 0); break;
        default: masked_units<uint8_t>(s, a.mask, a.batch, a.want != 0); break;
    }
}

}  // namespace

hipError_t vmas_aux::fill_u32_async(void* dst, uint32_t value, size_t n_words, hipStream_t stream) {
    if (n_words == 0) return hipSuccess;
    const int64_t n = (int64_t)n_words;
    const int gx = (int)std::min<int64_t>(1024, (n + kFillThreads - 1) / kFillThreads);
    hipLaunchKernelGGL(k_fill_u32, dim3(gx), dim3(kFillThreads), 0, stream, (uint32_t*)dst, value, n);
    return hipGetLastError();
}

// a span the launch can run: a copy, an increment (src NULL: whole floats) or a store (STORE64)
static bool span_ok(const VmasCopySpan& s) {
    if (s.nbytes == VMAS_COPY_STORE64) return s.dst && ((uintptr_t)s.dst & 7) == 0;
    return s.nbytes >= 0 && (s.nbytes == 0 || s.dst) && (s.src || (s.nbytes % 4 == 0 && ((uintptr_t)s.dst & 3) == 0));
}

extern "C" int32_t vmas_copy_spans(int32_t device, const VmasCopySpan* spans, int32_t n, void* stream) {
    if (n < 0 || (n > 0 && !spans) || device < 0) return vmas_aux::fail(VMAS_E_INVALID, "vmas_copy_spans: bad arguments");
    VMAS_AUX_HIP(hipSetDevice(device));
    for (int first = 0; first < n; first += VMAS_COPY_MAX_SPANS) {
        CopyArgs a{};
        a.n = 0;
        int64_t most = 0;  // units of the largest span (16-byte units: sets the grid)
        for (int i = first; i < std::min(n, first + VMAS_COPY_MAX_SPANS); ++i) {
            const VmasCopySpan& s = spans[i];
            if (!span_ok(s)) return vmas_aux::fail(VMAS_E_INVALID, "vmas_copy_spans: bad span %d", i);
            if (s.nbytes == 0 || (s.nbytes > 0 && s.src == s.dst)) continue;
            a.s[a.n++] = s;
            most = std::max<int64_t>(most, s.nbytes > 0 ? (s.nbytes + 15) / 16 : 1);
        }
        if (a.n == 0) continue;
        const int64_t per_block = (int64_t)kCopyThreads * kCopyUnroll;
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxCopyBlocks, (most + per_block - 1) / per_block));
        hipLaunchKernelGGL(k_copy_spans, dim3(gx, a.n), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
        VMAS_AUX_HIP(hipGetLastError());
    }
    return VMAS_OK;
}

extern "C" int32_t vmas_copy_spans_draw(int32_t device, const VmasCopySpan* spans, int32_t n_spans, int64_t numel,
                                        const VmasUniformColumn* cols, int32_t n_cols, uint64_t seed, uint64_t offset,
                                        const uint64_t* offset_dev, int32_t mode, int64_t u_snap_delta,
                                        uint64_t* increment, void* stream) {
    if (device < 0 || n_spans < 0 || n_spans > kMergedSpans || (n_spans > 0 && !spans) || n_cols <= 0 ||
        n_cols > kMergedCols || !cols || numel <= 0 || !increment || mode < 0 || mode > 3)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_copy_spans_draw: bad arguments");
    VMAS_AUX_HIP(hipSetDevice(device));
    static int max_blocks[64] = {0};
    if (device >= 64) return vmas_aux::fail(VMAS_E_INVALID, "vmas_copy_spans_draw: device %d", device);
    if (!max_blocks[device]) {
        hipDeviceProp_t prop;
        VMAS_AUX_HIP(hipGetDeviceProperties(&prop, device));
        max_blocks[device] = prop.multiProcessorCount * (prop.maxThreadsPerMultiProcessor / vmas_uniform::kThreads);
        if (max_blocks[device] <= 0) return vmas_aux::fail(VMAS_E_HIP, "vmas_copy_spans_draw: device properties");
    }
    int gx_draw = 0;
    unsigned long long inc = 0;
    vmas_uniform::grid_for(numel, max_blocks[device], &gx_draw, &inc);
    CopyDrawArgs a{};
    int n = 0;
    for (int i = 0; i < n_spans; ++i) {
        const VmasCopySpan& sp = spans[i];
        if (!span_ok(sp)) return vmas_aux::fail(VMAS_E_INVALID, "vmas_copy_spans_draw: bad span %d", i);
        if (sp.nbytes == 0 || (sp.nbytes > 0 && sp.src == sp.dst)) continue;
        a.s[n++] = sp;
    }
    for (int i = 0; i < n_cols; ++i) {
        if (!cols[i].out) return vmas_aux::fail(VMAS_E_INVALID, "vmas_copy_spans_draw: null column %d", i);
        a.c[i] = cols[i];
        a.c[i].offset = offset + inc * (unsigned long long)i;
    }
    a.seed = seed;
    a.numel = numel;
    a.snap = u_snap_delta;
    a.off_dev = reinterpret_cast<const unsigned long long*>(offset_dev);
    a.n_spans = n;
    a.gx_draw = gx_draw;
    a.mode = mode;
    const int64_t per_share = (int64_t)kCopyThreads * kCopyUnroll;
    a.n_items = n + n_cols;
    int total = 0;
    for (int y = 0; y < n + n_cols; ++y) {
        a.first[y] = total;
        if (y < n) {  // a span's own share: its 16-byte units over 256 threads x 4, at least one
            const VmasCopySpan& sp = a.s[y];
            const int64_t units = sp.nbytes > 0 ? (sp.nbytes + 15) / 16 : 1;
            total += (int)std::max<int64_t>(1, std::min<int64_t>(kMaxCopyBlocks, (units + per_share - 1) / per_share));
        } else {
            total += gx_draw;
        }
    }
    a.first[n + n_cols] = total;
    static int trace = getenv("VMAS_COPY_TRACE") ? atoi(getenv("VMAS_COPY_TRACE")) : 0;
    if (trace > 0) {  // (a diagnostic: the first calls' span list, to stderr)
        --trace;
        int64_t bytes = 0;
        for (int i = 0; i < n; ++i) bytes += a.s[i].nbytes > 0 ? a.s[i].nbytes : 0;
        fprintf(stderr, "[vmas_copy_spans_draw] spans %d cols %d numel %lld bytes %lld workgroups %d (%d per draw column)\n",
                n, n_cols, (long long)numel, (long long)bytes, total, gx_draw);
        for (int i = 0; i < n; ++i)
            fprintf(stderr, "  span %d: %lld bytes%s\n", i, (long long)a.s[i].nbytes, a.s[i].src ? "" : " (increment)");
    }
    hipLaunchKernelGGL(k_copy_draw, dim3((unsigned)total), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
    VMAS_AUX_HIP(hipGetLastError());
    *increment = inc * (unsigned long long)n_cols;
    return VMAS_OK;
}

extern "C" int32_t vmas_masked_rows(int32_t device, const VmasMaskedSpan* spans, int32_t n, const uint8_t* mask,
                                    int64_t batch, int32_t copy_if_set, void* stream) {
    if (n < 0 || (n > 0 && !spans) || batch < 0 || (batch > 0 && !mask) || device < -1)
        return vmas_aux::fail(VMAS_E_INVALID, "vmas_masked_rows: bad arguments");
    for (int i = 0; i < n; ++i) {
        const VmasMaskedSpan& s = spans[i];
        // (rows of one tensor must not overlap: a stride shorter than the row would make the result
        // depend on the order of the copies)
        if (s.row_bytes < 0 || (s.row_bytes > 0 && (!s.dst || !s.src)) || s.dst_stride < s.row_bytes ||
            s.src_stride < 0)
            return vmas_aux::fail(VMAS_E_INVALID, "vmas_masked_rows: bad span %d", i);
    }
    const bool want = copy_if_set != 0;
    if (device < 0) {  // the host backend: the same loop over host pointers
        for (int i = 0; i < n; ++i) {
            const VmasMaskedSpan& s = spans[i];
            if (s.row_bytes == 0) continue;
            for (int64_t b = 0; b < batch; ++b)
                if ((mask[b] != 0) == want)
                    memmove(static_cast<char*>(s.dst) + b * s.dst_stride, static_cast<const char*>(s.src) + b * s.src_stride,
                            (size_t)s.row_bytes);
        }
        return VMAS_OK;
    }
    if (batch == 0) return VMAS_OK;
    VMAS_AUX_HIP(hipSetDevice(device));
    for (int first = 0; first < n; first += VMAS_MASKED_MAX_SPANS) {
        MaskedArgs a{};
        int m = 0;
        int64_t most = 0;  // units of the largest span: sets the grid
        for (int i = first; i < std::min(n, first + VMAS_MASKED_MAX_SPANS); ++i) {
            const VmasMaskedSpan& s = spans[i];
            if (s.row_bytes == 0) continue;
            a.s[m++] = s;
            most = std::max<int64_t>(most, batch * (s.row_bytes / masked_unit(s)));
        }
        if (m == 0) continue;
        a.mask = mask;
        a.batch = batch;
        a.want = want ? 1 : 0;
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxCopyBlocks, (most + kCopyThreads - 1) / kCopyThreads));
        hipLaunchKernelGGL(k_masked_rows, dim3(gx, m), dim3(kCopyThreads), 0, (hipStream_t)stream, a);
        VMAS_AUX_HIP(hipGetLastError());
    }
    return VMAS_OK;
}
