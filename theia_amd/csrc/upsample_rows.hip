// Nearest-neighbour expansion of token rows and its adjoint: the spatial half of the MLP translator head
// (reference models/adapter_heads.py:96-102, F.interpolate(mode="nearest") on [b, C, hs, ws]) in the token-major layout
// the engine keeps, [b, h*w, C].  The MLP acts on each row alone, so the engine runs it on the hs*ws source rows and expands
// only its result; the backward reduces the gradient onto the source rows first.
//
// Index map (one axis; PyTorch's nearest_idx): identity when the sizes agree, i >> 1 when the output is twice the input,
// otherwise min(floor(i * (float)in / out), in - 1) with a float32 scale.  The map is monotone, so the preimage of a source
// index is a contiguous interval of output indices (empty when downsampling skips it); the backward finds its ends by
// bisection on the same function.
#include "common.h"

namespace {

struct Axis {
    int in, out;
    float scale;  // (float)in / (float)out, divided on the host (IEEE f32)
};

static Axis make_axis(int in, int out) { return Axis{in, out, (float)in / (float)out}; }

__device__ __forceinline__ int nearest_src(const Axis& a, int i) {
    if (a.out == a.in) return i;
    if (a.out == 2 * a.in) return i >> 1;
    const int s = (int)floorf((float)i * a.scale);
    return s < a.in - 1 ? s : a.in - 1;
}

// first output index i in [0, out] with nearest_src(i) >= s (out when there is none)
__device__ __forceinline__ int preimage_begin(const Axis& a, int s) {
    int lo = 0, hi = a.out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (nearest_src(a, mid) >= s) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// dst[b, y*wt + x, :] = src[b, hy(y)*ws + wx(x), :].  W = bytes per vector (16, or the element size for the scalar path);
// one thread per vector, grid-stride.  A pure copy of bit patterns.
template <typename V>
__global__ void __launch_bounds__(256) nearest_rows_fwd_kernel(const V* __restrict__ src, V* __restrict__ dst, int64_t nvec, int vpr,
                                                               int ws, Axis ay, Axis ax) {
    const int64_t hwt = (int64_t)ay.out * ax.out;
    const int64_t hws = (int64_t)ay.in * ws;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / vpr;
        const int v = (int)(i - row * vpr);
        const int64_t bi = row / hwt;
        const int p = (int)(row - bi * hwt);
        const int y = p / ax.out, x = p - y * ax.out;
        const int64_t srow = bi * hws + (int64_t)nearest_src(ay, y) * ws + nearest_src(ax, x);
        dst[i] = src[srow * vpr + v];
    }
}

// vectors of 16 bytes <-> f32 accumulators
template <typename T> struct Vec16;
template <> struct Vec16<bf16_t> {
    static constexpr int n = 8;
    __device__ static __forceinline__ void add(const bf16_t* p, float (&a)[8]) {
        float v[8];
        load8(p, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += v[j];
    }
    __device__ static __forceinline__ void store(bf16_t* p, const float (&a)[8]) { store8(p, a); }
};
template <> struct Vec16<float> {
    static constexpr int n = 4;
    __device__ static __forceinline__ void add(const float* p, float (&a)[4]) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
    }
    __device__ static __forceinline__ void store(float* p, const float (&a)[4]) { *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]); }
};

// dx[b, s, c] = sum over the preimage of s (y ascending, then x ascending) of dy[b, y*wt + x, c]; f32 sums, one rounding.
// One thread owns NV consecutive channels of one source row (a 16-byte vector, or one element on the scalar path) and writes
// them once: no atomics, a fixed order, bit-reproducible.  Zero where the preimage is empty.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) nearest_rows_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int64_t nthr, int tpr, int C,
                                                               int hs, int ws, Axis ay, Axis ax) {
    constexpr int NV = VEC ? Vec16<T>::n : 1;
    const int64_t hws = (int64_t)hs * ws;
    const int64_t hwt = (int64_t)ay.out * ax.out;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nthr; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / tpr;
        const int c = (int)(i - row * tpr) * NV;
        const int64_t bi = row / hws;
        const int p = (int)(row - bi * hws);
        const int sy = p / ws, sx = p - sy * ws;
        const int y0 = preimage_begin(ay, sy), y1 = preimage_begin(ay, sy + 1);
        const int x0 = preimage_begin(ax, sx), x1 = preimage_begin(ax, sx + 1);
        float a[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) a[j] = 0.f;
        const T* base = dy + bi * hwt * C + c;
        for (int y = y0; y < y1; ++y) {
            for (int x = x0; x < x1; ++x) {
                const T* q = base + ((int64_t)y * ax.out + x) * C;
                if constexpr (VEC) Vec16<T>::add(q, a);
                else a[0] += Elem<T>::ld(q);
            }
        }
        T* o = dx + row * C + c;
        if constexpr (VEC) Vec16<T>::store(o, a);
        else Elem<T>::st(o, a[0]);
    }
}

static int grid_of(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < 8192 ? (g > 0 ? g : 1) : 8192);
}

static bool overlaps(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// shared argument checks; on success *esz = element size
static int check_args(const char* who, const void* in, const void* out, int b, int hs, int ws, int ht, int wt, int C, int dtype,
                      bool fwd, int* esz) {
    THEIA_CHECK_ARG(in != nullptr && out != nullptr, "%s: null pointer", who);
    THEIA_CHECK_ARG(b > 0 && hs > 0 && ws > 0 && ht > 0 && wt > 0 && C > 0, "%s: sizes must be positive (b=%d hs=%d ws=%d ht=%d wt=%d C=%d)",
                    who, b, hs, ws, ht, wt, C);
    THEIA_CHECK_ARG(dtype == THEIA_F32 || dtype == THEIA_BF16, "%s: bad dtype %d", who, dtype);
    *esz = dtype == THEIA_F32 ? 4 : 2;
    const int64_t src_bytes = (int64_t)b * hs * ws * C * *esz, dst_bytes = (int64_t)b * ht * wt * C * *esz;
    THEIA_CHECK_ARG(!(fwd ? overlaps(in, src_bytes, out, dst_bytes) : overlaps(in, dst_bytes, out, src_bytes)),
                    "%s: output overlaps input", who);
    return THEIA_OK;
}

}  // namespace

extern "C" int theia_nearest_rows_fwd(const void* src, void* dst, int b, int hs, int ws, int ht, int wt, int C, int dtype, void* stream) {
    int esz = 0;
    const int rc = check_args("theia_nearest_rows_fwd", src, dst, b, hs, ws, ht, wt, C, dtype, true, &esz);
    if (rc != THEIA_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Axis ay = make_axis(hs, ht), ax = make_axis(ws, wt);
    const int64_t rows = (int64_t)b * ht * wt;
    const int64_t row_bytes = (int64_t)C * esz;
    if (row_bytes % 16 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0) {
        const int vpr = (int)(row_bytes / 16);
        hipLaunchKernelGGL(nearest_rows_fwd_kernel<uint4>, dim3(grid_of(rows * vpr)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst,
                           rows * vpr, vpr, ws, ay, ax);
    } else if (esz == 4) {
        hipLaunchKernelGGL(nearest_rows_fwd_kernel<uint32_t>, dim3(grid_of(rows * C)), dim3(256), 0, s, (const uint32_t*)src, (uint32_t*)dst,
                           rows * C, C, ws, ay, ax);
    } else {
        hipLaunchKernelGGL(nearest_rows_fwd_kernel<uint16_t>, dim3(grid_of(rows * C)), dim3(256), 0, s, (const uint16_t*)src, (uint16_t*)dst,
                           rows * C, C, ws, ay, ax);
    }
    THEIA_CHECK_LAUNCH("theia_nearest_rows_fwd");
    return THEIA_OK;
}

extern "C" int theia_nearest_rows_bwd(const void* dy, void* dx, int b, int hs, int ws, int ht, int wt, int C, int dtype, void* stream) {
    int esz = 0;
    const int rc = check_args("theia_nearest_rows_bwd", dy, dx, b, hs, ws, ht, wt, C, dtype, false, &esz);
    if (rc != THEIA_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Axis ay = make_axis(hs, ht), ax = make_axis(ws, wt);
    const int64_t rows = (int64_t)b * hs * ws;
    const bool vec = ((int64_t)C * esz) % 16 == 0 && ((uintptr_t)dy | (uintptr_t)dx) % 16 == 0;
    const int per = vec ? 16 / esz : 1;
    const int tpr = C / per;
    const int g = grid_of(rows * tpr);
    if (esz == 2) {
        if (vec) hipLaunchKernelGGL((nearest_rows_bwd_kernel<bf16_t, true>), dim3(g), dim3(256), 0, s, (const bf16_t*)dy, (bf16_t*)dx, rows * tpr, tpr, C, hs, ws, ay, ax);
        else hipLaunchKernelGGL((nearest_rows_bwd_kernel<bf16_t, false>), dim3(g), dim3(256), 0, s, (const bf16_t*)dy, (bf16_t*)dx, rows * tpr, tpr, C, hs, ws, ay, ax);
    } else {
        if (vec) hipLaunchKernelGGL((nearest_rows_bwd_kernel<float, true>), dim3(g), dim3(256), 0, s, (const float*)dy, (float*)dx, rows * tpr, tpr, C, hs, ws, ay, ax);
        else hipLaunchKernelGGL((nearest_rows_bwd_kernel<float, false>), dim3(g), dim3(256), 0, s, (const float*)dy, (float*)dx, rows * tpr, tpr, C, hs, ws, ay, ax);
    }
    THEIA_CHECK_LAUNCH("theia_nearest_rows_bwd");
    return THEIA_OK;
}
