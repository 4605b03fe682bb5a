// K4 (long sequences): key-tiled ("flash") multi-head self-attention forward / backward, head_dim = 64, any n <= TL_MAXN.
//
// The kernels of attention.hip / attention_mfma.hip keep a whole (image, head) sequence in LDS and stop at n = 256.  Here a
// workgroup owns a 64-row block of ONE (image, head): 4 wave64, each wave a 16-row query (resp. key) tile held in registers, and
// the other side of the product streams through LDS in 64-row chunks.  Grid: one workgroup per (image, head, 64-row block), the
// blocks of a head adjacent (they read the same K / V, resp. Q / dO, out of L2).  Every address is 64-bit; nothing is atomic, every
// sum runs in a fixed order (the gradients are bit-reproducible).
//
// bf16 (matrix cores, v_mfma_f32_16x16x32_bf16; the operand layout of attention_mfma.hip: scores computed transposed so a lane owns
// one query (resp. key) row and 4 consecutive keys (resp. queries) per 16-row tile, the second operand of the P V / dS K / P^T dO /
// dS^T Q products read through ds_read_b64_tr_b16 with the same k-slot permutation):
//   attn_tiled_fwd_bf16_kernel   K / V chunks double-buffered in LDS (the next chunk is requested into registers before the current
//                                one is used, written to the other buffer behind it: one barrier per chunk), online softmax in f32
//   attn_tiled_dq_bf16_kernel    K / V chunks as in the forward; P recomputed from lse, dQ = dS K
//   attn_tiled_dkv_bf16_kernel   Q / dO chunks (+ their lse / delta rows) double-buffered; dV = P^T dO, dK = dS^T Q
//   LDS 36 KB (dQ / forward), 37 KB (dK dV): four workgroups per CU -> designed for 4 waves per SIMD, <= 128 VGPRs.
// f32 (VALU, exact "parity" precision; the arithmetic of the kernels in attention.hip, tiled the same way, one chunk per barrier pair):
//   attn_tiled_fwd_f32_kernel    a wave walks its 16 query rows per chunk, lanes over the chunk's 64 keys, then over the 64 d
//   attn_tiled_dq_f32_kernel / attn_tiled_dkv_f32_kernel   the same for the two halves of the backward
//   LDS 52 KB (forward): three workgroups per CU -> designed for 3 waves per SIMD, <= 168 VGPRs; 69 / 70.5 KB (dQ / dK dV): two
//   workgroups per CU -> 2 waves per SIMD, <= 256 VGPRs.
// attn_tiled_delta_kernel<T>: delta = rowsum(dO o O) into the backward's workspace (f32 [b, h, n]), 8 lanes per row.
//
// Tails: keys >= n get probability exactly 0 (score masked to -inf in the forward and dQ kernels, P selected to 0 in the dK dV
// kernel); staged rows beyond n are zeros; query (resp. key) rows >= n are never stored.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 tl_bf16x8;
typedef __attribute__((ext_vector_type(4))) float tl_f32x4;
typedef __attribute__((ext_vector_type(4))) short tl_s16x4;

constexpr int TL_MAXN = 8192;    // longest sequence accepted (a 1024x1024 input with register tokens is 4104)
constexpr int TL_ROWS = 64;      // rows per workgroup block and per streamed chunk
constexpr int TL_THREADS = 256;  // 4 wave64, one 16-row tile each
constexpr int TL_PITCH = 144;    // bf16 LDS row: 64 bf16 + 16 B pad (16 rows of a fragment read hit 16 distinct bank slots)
constexpr int TL_FPITCH = 68;    // f32 LDS row: 64 floats + 4 pad (conflict-free 16-byte reads)
constexpr int TL_CHUNK_B = TL_ROWS * TL_PITCH;
constexpr float TL_C = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e): exp(x/8 - m) = exp2(x*TL_C - m*log2e)
constexpr float TL_LOG2E = 1.4426950408889634f;

// ------------------------------------------------------------------------------------------------ bf16 helpers
__device__ __forceinline__ void tl_mma(tl_f32x4& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tl_bf16x8, a), __builtin_bit_cast(tl_bf16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ uint4 tl_keep(bool c, const uint4& a) { return make_uint4(c ? a.x : 0u, c ? a.y : 0u, c ? a.z : 0u, c ? a.w : 0u); }
// natural fragment: row (row0 + lane&15), d = kk*32 + (lane>>4)*8 .. +8
__device__ __forceinline__ uint4 tl_nat(const char* __restrict__ base, int row0, int kk, int lane) {
    return *reinterpret_cast<const uint4*>(base + (row0 + (lane & 15)) * TL_PITCH + (kk * 4 + (lane >> 4)) * 16);
}
// transposed fragment: column d = df*16 + (lane&15); rows 32s + 4g + {0..3} and 32s + 16 + 4g + {0..3}
__device__ __forceinline__ uint4 tl_tr(const char* __restrict__ base, int s, int df, int lane) {
    const int q = lane & 15, g = lane >> 4;
    const char* p = base + (s * 32 + g * 4 + (q >> 2)) * TL_PITCH + (df * 16 + (q & 3) * 4) * 2;
    const tl_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tl_s16x4*)(p));
    const tl_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tl_s16x4*)(p + 16 * TL_PITCH));
    const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
    return make_uint4(l2.x, l2.y, h2.x, h2.y);
}
__device__ __forceinline__ uint4 tl_pack(const tl_f32x4& t0, const tl_f32x4& t1) {
    return make_uint4(pack2_bf16(t0[0], t0[1]), pack2_bf16(t0[2], t0[3]), pack2_bf16(t1[0], t1[1]), pack2_bf16(t1[2], t1[3]));
}
__device__ __forceinline__ float tl_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32 (arguments <= 0 or -inf)
__device__ __forceinline__ float tl_rsum(float v) {  // over the 4 lane groups (lanes l, l^16, l^32, l^48)
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float tl_rmax(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}
__device__ __forceinline__ void tl_store4(bf16_t* p, const tl_f32x4& v, float scale) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack2_bf16(v[0] * scale, v[1] * scale), pack2_bf16(v[2] * scale, v[3] * scale));
}

// A 64-row chunk of two [token][64] bf16 matrices: requested into registers (unconditional loads from rows clamped into [0, n); a
// load under a lane mask is a branch, and the compiler drains the memory counter where its sides meet), later written to LDS with
// rows beyond n as zeros.
struct TlChunk {
    uint4 a[2], b[2];
};
__device__ __forceinline__ void tl_request(TlChunk& x, const bf16_t* __restrict__ srcA, int64_t strideA, const bf16_t* __restrict__ srcB,
                                           int64_t strideB, int row0, int n) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int v = threadIdx.x + it * TL_THREADS, r = min(row0 + (v >> 3), n - 1), c = v & 7;
        x.a[it] = *reinterpret_cast<const uint4*>(srcA + r * strideA + c * 8);
        x.b[it] = *reinterpret_cast<const uint4*>(srcB + r * strideB + c * 8);
    }
}
__device__ __forceinline__ void tl_commit(const TlChunk& x, char* __restrict__ dA, char* __restrict__ dB, int row0, int n) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int v = threadIdx.x + it * TL_THREADS, r = v >> 3, c = v & 7;
        const bool live = row0 + r < n;
        *reinterpret_cast<uint4*>(dA + r * TL_PITCH + c * 16) = tl_keep(live, x.a[it]);
        *reinterpret_cast<uint4*>(dB + r * TL_PITCH + c * 16) = tl_keep(live, x.b[it]);
    }
}

// ================================================================================================ bf16 forward
__global__ __launch_bounds__(TL_THREADS) void attn_tiled_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o,
                                                                         float* __restrict__ lse, int n, int h, int nblk) {
    __shared__ __attribute__((aligned(16))) char sm[2][2][TL_CHUNK_B];  // [buffer][K, V][64 rows]
    const int bh = blockIdx.x / nblk, blk = blockIdx.x % nblk, bi = bh / h, hi = bh % h;
    const int D = h * 64;
    const int64_t rs = 3 * (int64_t)D;
    const bf16_t* base = qkv + (int64_t)bi * n * rs + hi * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q16 = lane & 15, g = lane >> 4;
    const int qrow = blk * TL_ROWS + wave * 16 + q16;
    const bool qok = qrow < n;
    uint4 qf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[kk] = *reinterpret_cast<const uint4*>(base + min(qrow, n - 1) * rs + kk * 32 + g * 8);
    TlChunk x;
    tl_request(x, base + D, rs, base + 2 * D, rs, 0, n);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[kk] = tl_keep(qok, qf[kk]);
    tl_commit(x, sm[0][0], sm[0][1], 0, n);
    __syncthreads();
    float m = -INFINITY, l = 0.f;  // running max of the raw scores q.k (the row's, identical in the 4 lane groups); lane-partial sum
    tl_f32x4 oa[4];
#pragma unroll
    for (int df = 0; df < 4; ++df) oa[df] = (tl_f32x4){0.f, 0.f, 0.f, 0.f};
    const int nch = (n + TL_ROWS - 1) / TL_ROWS;
    for (int c = 0; c < nch; ++c) {
        const int k0 = c * TL_ROWS;
        const bool more = c + 1 < nch;
        if (more) tl_request(x, base + D, rs, base + 2 * D, rs, k0 + TL_ROWS, n);
        const char* sK = sm[c & 1][0];
        const char* sV = sm[c & 1][1];
        tl_f32x4 s[4];
        float cm = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            tl_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            tl_mma(acc, tl_nat(sK, kt * 16, 0, lane), qf[0]);
            tl_mma(acc, tl_nat(sK, kt * 16, 1, lane), qf[1]);
            if (k0 + TL_ROWS > n) {  // the last chunk straddles n: its keys beyond n get probability 0
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = k0 + kt * 16 + g * 4 + r < n ? acc[r] : -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) cm = fmaxf(cm, acc[r]);
            s[kt] = acc;
        }
        // every chunk holds at least one key < n, so mn is finite; in the first chunk m = -inf and alpha = exp2(-inf) = 0
        const float mn = fmaxf(m, tl_rmax(cm));
        const float alpha = tl_exp2((m - mn) * TL_C);
        const float mc = mn * TL_C;
        float cs = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = tl_exp2(fmaf(s[kt][r], TL_C, -mc));
                s[kt][r] = p;
                cs += p;
            }
        l = fmaf(l, alpha, cs);
        m = mn;
#pragma unroll
        for (int df = 0; df < 4; ++df) oa[df] *= alpha;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const uint4 pb = tl_pack(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
            for (int df = 0; df < 4; ++df) tl_mma(oa[df], tl_tr(sV, ks, df, lane), pb);
        }
        if (more) tl_commit(x, sm[(c + 1) & 1][0], sm[(c + 1) & 1][1], k0 + TL_ROWS, n);
        __syncthreads();
    }
    l = tl_rsum(l);
    if (qok) {
        const float inv = 1.0f / l;
        bf16_t* orow = o + ((int64_t)bi * n + qrow) * D + hi * 64 + g * 4;
#pragma unroll
        for (int df = 0; df < 4; ++df) tl_store4(orow + df * 16, oa[df], inv);
        if (g == 0) lse[(int64_t)bh * n + qrow] = m * 0.125f + __logf(l);
    }
}

// ================================================================================================ backward: delta
// delta[b, h, i] = sum_d dO[b, i, h*64 + d] * O[b, i, h*64 + d]; o / dO are [b*n*h] rows of 64 in (image, token, head) order
template <typename T>
__global__ __launch_bounds__(TL_THREADS) void attn_tiled_delta_kernel(const T* __restrict__ o, const T* __restrict__ d_o,
                                                                      float* __restrict__ delta, int n, int h, int64_t rows) {
    const int64_t r = (int64_t)blockIdx.x * (TL_THREADS / 8) + (threadIdx.x >> 3);
    const int c = threadIdx.x & 7;
    float part = 0.f;
    if (r < rows) {
        float a[8], b[8];
        load8(d_o + r * 64 + c * 8, a);
        load8(o + r * 64 + c * 8, b);
#pragma unroll
        for (int j = 0; j < 8; ++j) part += a[j] * b[j];
    }
    part += __shfl_xor(part, 1, 64);
    part += __shfl_xor(part, 2, 64);
    part += __shfl_xor(part, 4, 64);
    if (r < rows && c == 0) {
        const int hi = (int)(r % h);
        const int64_t t = r / h;
        const int i = (int)(t % n);
        const int64_t bi = t / n;
        delta[(bi * h + hi) * n + i] = part;
    }
}

// ================================================================================================ bf16 backward: dQ
__global__ __launch_bounds__(TL_THREADS) void attn_tiled_dq_bf16_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ d_o,
                                                                        const float* __restrict__ lse, const float* __restrict__ delta,
                                                                        bf16_t* __restrict__ dqkv, int n, int h, int nblk) {
    __shared__ __attribute__((aligned(16))) char sm[2][2][TL_CHUNK_B];  // [buffer][K, V][64 rows]
    const int bh = blockIdx.x / nblk, blk = blockIdx.x % nblk, bi = bh / h, hi = bh % h;
    const int D = h * 64;
    const int64_t rs = 3 * (int64_t)D;
    const bf16_t* base = qkv + (int64_t)bi * n * rs + hi * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q16 = lane & 15, g = lane >> 4;
    const int qrow = blk * TL_ROWS + wave * 16 + q16;
    const bool qok = qrow < n;
    const int qc = min(qrow, n - 1);
    uint4 qf[2], gf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        qf[kk] = *reinterpret_cast<const uint4*>(base + qc * rs + kk * 32 + g * 8);
        gf[kk] = *reinterpret_cast<const uint4*>(d_o + ((int64_t)bi * n + qc) * D + hi * 64 + kk * 32 + g * 8);
    }
    const float lq = lse[(int64_t)bh * n + qc], dq_delta = delta[(int64_t)bh * n + qc];
    TlChunk x;
    tl_request(x, base + D, rs, base + 2 * D, rs, 0, n);
    // query rows beyond n: zero Q / dO, lse and delta 0 -> P = 1, dS = 0 (finite, never stored)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        qf[kk] = tl_keep(qok, qf[kk]);
        gf[kk] = tl_keep(qok, gf[kk]);
    }
    const float lq2 = qok ? lq * TL_LOG2E : 0.f, dl = qok ? dq_delta : 0.f;
    tl_commit(x, sm[0][0], sm[0][1], 0, n);
    __syncthreads();
    tl_f32x4 dq[4];
#pragma unroll
    for (int df = 0; df < 4; ++df) dq[df] = (tl_f32x4){0.f, 0.f, 0.f, 0.f};
    const int nch = (n + TL_ROWS - 1) / TL_ROWS;
    for (int c = 0; c < nch; ++c) {
        const int k0 = c * TL_ROWS;
        const bool more = c + 1 < nch;
        if (more) tl_request(x, base + D, rs, base + 2 * D, rs, k0 + TL_ROWS, n);
        const char* sK = sm[c & 1][0];
        const char* sV = sm[c & 1][1];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            tl_f32x4 dsv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kt = 2 * ks + t;
                tl_f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                tl_mma(st, tl_nat(sK, kt * 16, 0, lane), qf[0]);
                tl_mma(st, tl_nat(sK, kt * 16, 1, lane), qf[1]);
                tl_mma(dp, tl_nat(sV, kt * 16, 0, lane), gf[0]);
                tl_mma(dp, tl_nat(sV, kt * 16, 1, lane), gf[1]);
                if (k0 + TL_ROWS > n) {  // keys beyond n: probability 0
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[r] = k0 + kt * 16 + g * 4 + r < n ? st[r] : -INFINITY;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) dsv[t][r] = tl_exp2(fmaf(st[r], TL_C, -lq2)) * (dp[r] - dl) * 0.125f;
            }
            const uint4 sb = tl_pack(dsv[0], dsv[1]);
#pragma unroll
            for (int df = 0; df < 4; ++df) tl_mma(dq[df], tl_tr(sK, ks, df, lane), sb);
        }
        if (more) tl_commit(x, sm[(c + 1) & 1][0], sm[(c + 1) & 1][1], k0 + TL_ROWS, n);
        __syncthreads();
    }
    if (qok) {
        bf16_t* drow = dqkv + ((int64_t)bi * n + qrow) * rs + hi * 64 + g * 4;
#pragma unroll
        for (int df = 0; df < 4; ++df) tl_store4(drow + df * 16, dq[df], 1.0f);
    }
}

// ================================================================================================ bf16 backward: dK, dV
// (amdgpu_waves_per_eu(4): left to itself the compiler takes 136 registers -- 3 waves per SIMD -- for 8 it does not need)
__global__ __launch_bounds__(TL_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void attn_tiled_dkv_bf16_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ d_o,
                                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                                         bf16_t* __restrict__ dqkv, int n, int h, int nblk) {
    __shared__ __attribute__((aligned(16))) char sm[2][2][TL_CHUNK_B];   // [buffer][Q, dO][64 rows]
    __shared__ __attribute__((aligned(16))) float sLD[2][2][TL_ROWS];   // [buffer][lse * log2e (+inf beyond n), delta (0 beyond n)]
    const int bh = blockIdx.x / nblk, blk = blockIdx.x % nblk, bi = bh / h, hi = bh % h;
    const int D = h * 64;
    const int64_t rs = 3 * (int64_t)D;
    const bf16_t* base = qkv + (int64_t)bi * n * rs + hi * 64;
    const bf16_t* gbase = d_o + (int64_t)bi * n * D + hi * 64;
    const float* lrow = lse + (int64_t)bh * n;
    const float* drow_ = delta + (int64_t)bh * n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k16 = lane & 15, g = lane >> 4;
    const int krow = blk * TL_ROWS + wave * 16 + k16;
    const bool kok = krow < n;
    const int kc = min(krow, n - 1);
    uint4 kf[2], vf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        kf[kk] = *reinterpret_cast<const uint4*>(base + kc * rs + D + kk * 32 + g * 8);
        vf[kk] = *reinterpret_cast<const uint4*>(base + kc * rs + 2 * D + kk * 32 + g * 8);
    }
    TlChunk x;
    float xl, xd;  // threads < 64: one lse / delta row of the chunk
    auto request = [&](int q0) {
        tl_request(x, base, rs, gbase, (int64_t)D, q0, n);
        const int r = min(q0 + (int)(threadIdx.x & 63), n - 1);
        xl = lrow[r];
        xd = drow_[r];
    };
    auto commit = [&](int buf, int q0) {
        tl_commit(x, sm[buf][0], sm[buf][1], q0, n);
        if (threadIdx.x < TL_ROWS) {
            const bool live = q0 + (int)threadIdx.x < n;
            sLD[buf][0][threadIdx.x] = live ? xl * TL_LOG2E : INFINITY;  // P = exp2(finite - inf) = 0
            sLD[buf][1][threadIdx.x] = live ? xd : 0.f;
        }
    };
    request(0);
    commit(0, 0);
    __syncthreads();
    tl_f32x4 dk[4], dv[4];
#pragma unroll
    for (int df = 0; df < 4; ++df) dk[df] = dv[df] = (tl_f32x4){0.f, 0.f, 0.f, 0.f};
    const int nch = (n + TL_ROWS - 1) / TL_ROWS;
    for (int c = 0; c < nch; ++c) {
        const int q0c = c * TL_ROWS;
        const bool more = c + 1 < nch;
        if (more) request(q0c + TL_ROWS);
        const char* sQ = sm[c & 1][0];
        const char* sG = sm[c & 1][1];
        const float* sL = sLD[c & 1][0];
        const float* sD = sLD[c & 1][1];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            tl_f32x4 p[2], dsv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int q0 = (2 * ks + t) * 16;
                tl_f32x4 sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
                tl_mma(sa, tl_nat(sQ, q0, 0, lane), kf[0]);
                tl_mma(sa, tl_nat(sQ, q0, 1, lane), kf[1]);
                tl_mma(da, tl_nat(sG, q0, 0, lane), vf[0]);
                tl_mma(da, tl_nat(sG, q0, 1, lane), vf[1]);
                const float4 l4 = *reinterpret_cast<const float4*>(sL + q0 + g * 4), d4 = *reinterpret_cast<const float4*>(sD + q0 + g * 4);
                const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // a key beyond n (clamped row, its column never stored) is selected to 0 all the same: exp2 of its score against a
                    // very negative lse can overflow
                    const float pv = kok ? tl_exp2(fmaf(sa[r], TL_C, -lq[r])) : 0.f;
                    p[t][r] = pv;
                    dsv[t][r] = pv * (da[r] - dl[r]) * 0.125f;
                }
            }
            const uint4 pb = tl_pack(p[0], p[1]), sb = tl_pack(dsv[0], dsv[1]);
#pragma unroll
            for (int df = 0; df < 4; ++df) {
                tl_mma(dv[df], tl_tr(sG, ks, df, lane), pb);
                tl_mma(dk[df], tl_tr(sQ, ks, df, lane), sb);
            }
        }
        if (more) commit((c + 1) & 1, q0c + TL_ROWS);
        __syncthreads();
    }
    if (kok) {
        bf16_t* drow = dqkv + ((int64_t)bi * n + krow) * rs + hi * 64 + g * 4;
#pragma unroll
        for (int df = 0; df < 4; ++df) {
            tl_store4(drow + D + df * 16, dk[df], 1.0f);
            tl_store4(drow + 2 * D + df * 16, dv[df], 1.0f);
        }
    }
}

// ================================================================================================ f32 kernels
// `rows` rows (64 floats each, row r at src + r*stride) starting at token row0 -> dst[r][0..63], zero beyond n
__device__ __forceinline__ void tl_stage_f32(const float* __restrict__ src, int64_t stride, int row0, int n, float* __restrict__ dst) {
    for (int v = threadIdx.x; v < TL_ROWS * 16; v += TL_THREADS) {
        const int r = v >> 4, c = (v & 15) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < n) x = *reinterpret_cast<const float4*>(src + (row0 + r) * stride + c);
        *reinterpret_cast<float4*>(dst + r * TL_FPITCH + c) = x;
    }
}
__device__ __forceinline__ float tl_dot64(const float* __restrict__ a, const float* __restrict__ b) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + c);
        const float4 y = *reinterpret_cast<const float4*>(b + c);
        acc += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    return acc;
}

__global__ __launch_bounds__(TL_THREADS) void attn_tiled_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                                        float* __restrict__ lse, int n, int h, int nblk) {
    __shared__ __attribute__((aligned(16))) float sQ[TL_ROWS * TL_FPITCH];  // the block's query rows
    __shared__ __attribute__((aligned(16))) float sK[TL_ROWS * TL_FPITCH];  // the chunk's keys
    __shared__ __attribute__((aligned(16))) float sV[TL_ROWS * TL_FPITCH];
    __shared__ __attribute__((aligned(16))) float sP[4][TL_ROWS];
    const int bh = blockIdx.x / nblk, blk = blockIdx.x % nblk, bi = bh / h, hi = bh % h;
    const int D = h * 64;
    const int64_t rs = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)bi * n * rs + hi * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blk * TL_ROWS;
    tl_stage_f32(base, rs, r0, n, sQ);
    float m[16], l[16], acc[16];  // per query row of the wave: running max / sum (wave-uniform), o[row][lane]
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) m[rr] = -INFINITY, l[rr] = 0.f, acc[rr] = 0.f;
    float* myP = sP[wave];
    for (int k0 = 0; k0 < n; k0 += TL_ROWS) {
        __syncthreads();  // the previous chunk is no longer read
        tl_stage_f32(base + D, rs, k0, n, sK);
        tl_stage_f32(base + 2 * D, rs, k0, n, sV);
        __syncthreads();
        const bool kok = k0 + lane < n;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const float s = kok ? tl_dot64(sQ + (wave * 16 + rr) * TL_FPITCH, sK + lane * TL_FPITCH) * 0.125f : -INFINITY;
            const float mn = fmaxf(m[rr], wave_max(s));  // finite: key k0 < n
            const float alpha = expf(m[rr] - mn);
            const float p = expf(s - mn);
            l[rr] = l[rr] * alpha + wave_sum(p);
            m[rr] = mn;
            myP[lane] = p;
            __builtin_amdgcn_wave_barrier();
            float a = 0.f;
#pragma unroll 8
            for (int j = 0; j < TL_ROWS; ++j) a += myP[j] * sV[j * TL_FPITCH + lane];
            acc[rr] = acc[rr] * alpha + a;
            __builtin_amdgcn_wave_barrier();
        }
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int i = r0 + wave * 16 + rr;
        if (i < n) {
            o[((int64_t)bi * n + i) * D + hi * 64 + lane] = acc[rr] / l[rr];
            if (lane == 0) lse[(int64_t)bh * n + i] = m[rr] + logf(l[rr]);
        }
    }
}

__global__ __launch_bounds__(TL_THREADS) void attn_tiled_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                                       float* __restrict__ dqkv, int n, int h, int nblk) {
    __shared__ __attribute__((aligned(16))) float sQ[TL_ROWS * TL_FPITCH];  // the block's query rows
    __shared__ __attribute__((aligned(16))) float sG[TL_ROWS * TL_FPITCH];  // ... and their dO rows
    __shared__ __attribute__((aligned(16))) float sK[TL_ROWS * TL_FPITCH];  // the chunk's keys
    __shared__ __attribute__((aligned(16))) float sV[TL_ROWS * TL_FPITCH];
    __shared__ __attribute__((aligned(16))) float sS[4][TL_ROWS];
    const int bh = blockIdx.x / nblk, blk = blockIdx.x % nblk, bi = bh / h, hi = bh % h;
    const int D = h * 64;
    const int64_t rs = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)bi * n * rs + hi * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blk * TL_ROWS;
    tl_stage_f32(base, rs, r0, n, sQ);
    tl_stage_f32(d_o + (int64_t)bi * n * D + hi * 64, (int64_t)D, r0, n, sG);
    float lq[16], dl[16], acc[16];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int i = r0 + wave * 16 + rr;
        lq[rr] = i < n ? lse[(int64_t)bh * n + i] : 0.f;
        dl[rr] = i < n ? delta[(int64_t)bh * n + i] : 0.f;
        acc[rr] = 0.f;
    }
    float* myS = sS[wave];
    for (int k0 = 0; k0 < n; k0 += TL_ROWS) {
        __syncthreads();
        tl_stage_f32(base + D, rs, k0, n, sK);
        tl_stage_f32(base + 2 * D, rs, k0, n, sV);
        __syncthreads();
        const bool kok = k0 + lane < n;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const float* qr = sQ + (wave * 16 + rr) * TL_FPITCH;
            const float* gr = sG + (wave * 16 + rr) * TL_FPITCH;
            float ds = 0.f;
            if (kok) {
                const float p = expf(tl_dot64(qr, sK + lane * TL_FPITCH) * 0.125f - lq[rr]);
                ds = p * (tl_dot64(gr, sV + lane * TL_FPITCH) - dl[rr]) * 0.125f;
            }
            myS[lane] = ds;
            __builtin_amdgcn_wave_barrier();
            float a = 0.f;
#pragma unroll 8
            for (int j = 0; j < TL_ROWS; ++j) a += myS[j] * sK[j * TL_FPITCH + lane];
            acc[rr] += a;
            __builtin_amdgcn_wave_barrier();
        }
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int i = r0 + wave * 16 + rr;
        if (i < n) dqkv[((int64_t)bi * n + i) * rs + hi * 64 + lane] = acc[rr];
    }
}

__global__ __launch_bounds__(TL_THREADS) void attn_tiled_dkv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                        const float* __restrict__ lse, const float* __restrict__ delta,
                                                                        float* __restrict__ dqkv, int n, int h, int nblk) {
    __shared__ __attribute__((aligned(16))) float sK[TL_ROWS * TL_FPITCH];  // the block's key rows
    __shared__ __attribute__((aligned(16))) float sV[TL_ROWS * TL_FPITCH];
    __shared__ __attribute__((aligned(16))) float sQ[TL_ROWS * TL_FPITCH];  // the chunk's query rows
    __shared__ __attribute__((aligned(16))) float sG[TL_ROWS * TL_FPITCH];  // ... and their dO rows
    __shared__ float sL[TL_ROWS], sD[TL_ROWS];
    __shared__ __attribute__((aligned(16))) float sP[4][TL_ROWS];
    __shared__ __attribute__((aligned(16))) float sS[4][TL_ROWS];
    const int bh = blockIdx.x / nblk, blk = blockIdx.x % nblk, bi = bh / h, hi = bh % h;
    const int D = h * 64;
    const int64_t rs = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)bi * n * rs + hi * 64;
    const float* gbase = d_o + (int64_t)bi * n * D + hi * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blk * TL_ROWS;
    tl_stage_f32(base + D, rs, r0, n, sK);
    tl_stage_f32(base + 2 * D, rs, r0, n, sV);
    float ak[16], av[16];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) ak[rr] = av[rr] = 0.f;
    float* myP = sP[wave];
    float* myS = sS[wave];
    for (int q0 = 0; q0 < n; q0 += TL_ROWS) {
        __syncthreads();
        tl_stage_f32(base, rs, q0, n, sQ);
        tl_stage_f32(gbase, (int64_t)D, q0, n, sG);
        if (threadIdx.x < TL_ROWS) {
            const int i = q0 + threadIdx.x;
            sL[threadIdx.x] = i < n ? lse[(int64_t)bh * n + i] : 0.f;
            sD[threadIdx.x] = i < n ? delta[(int64_t)bh * n + i] : 0.f;
        }
        __syncthreads();
        const bool qok = q0 + lane < n;
        const float li = sL[lane], di = sD[lane];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const float* kr = sK + (wave * 16 + rr) * TL_FPITCH;
            const float* vr = sV + (wave * 16 + rr) * TL_FPITCH;
            float p = 0.f, ds = 0.f;
            if (qok && r0 + wave * 16 + rr < n) {
                p = expf(tl_dot64(kr, sQ + lane * TL_FPITCH) * 0.125f - li);
                ds = p * (tl_dot64(vr, sG + lane * TL_FPITCH) - di) * 0.125f;
            }
            myP[lane] = p;
            myS[lane] = ds;
            __builtin_amdgcn_wave_barrier();
            float a = 0.f, b = 0.f;
#pragma unroll 8
            for (int i = 0; i < TL_ROWS; ++i) {
                a += myP[i] * sG[i * TL_FPITCH + lane];
                b += myS[i] * sQ[i * TL_FPITCH + lane];
            }
            av[rr] += a;
            ak[rr] += b;
            __builtin_amdgcn_wave_barrier();
        }
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int j = r0 + wave * 16 + rr;
        if (j < n) {
            float* drow = dqkv + ((int64_t)bi * n + j) * rs + hi * 64 + lane;
            drow[D] = ak[rr];
            drow[2 * D] = av[rr];
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers (called from attention.hip)
static bool tl_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x + na <= y || y + nb <= x;
}

static int tl_check(const char* who, int b, int n, int h) {
    THEIA_CHECK_ARG(n <= TL_MAXN, "%s: n=%d must be in [1,%d]", who, n, TL_MAXN);
    // one workgroup per (image, head, 64-row block) in a 1-D grid; the delta kernel's rows are counted in 64 bits
    THEIA_CHECK_ARG((int64_t)b * h * ((n + TL_ROWS - 1) / TL_ROWS) <= INT32_MAX, "%s: b*h*ceil(n/64) = %lld workgroups exceed the grid", who,
                    (long long)b * h * ((n + TL_ROWS - 1) / TL_ROWS));
    return THEIA_OK;
}

int theia_attention_fwd_tiled(const void* qkv, void* o, float* lse, int b, int n, int h, int dtype, hipStream_t s) {
    const int rc = tl_check("theia_attention_fwd", b, n, h);
    if (rc != THEIA_OK) return rc;
    // other workgroups still read the K / V rows of a head while one writes its output: no output may overlap the input
    const size_t es = dtype == THEIA_BF16 ? 2 : 4, nq = (size_t)b * n * h * 64 * es, nl = (size_t)b * n * h * sizeof(float);
    THEIA_CHECK_ARG(tl_disjoint(o, nq, qkv, 3 * nq) && tl_disjoint(lse, nl, qkv, 3 * nq) && tl_disjoint(lse, nl, o, nq),
                    "theia_attention_fwd(b=%d, n=%d, h=%d): o / lse overlap qkv or each other", b, n, h);
    const int nblk = (n + TL_ROWS - 1) / TL_ROWS;
    const dim3 grid(b * h * nblk);
    if (dtype == THEIA_BF16)
        hipLaunchKernelGGL(attn_tiled_fwd_bf16_kernel, grid, dim3(TL_THREADS), 0, s, (const bf16_t*)qkv, (bf16_t*)o, lse, n, h, nblk);
    else
        hipLaunchKernelGGL(attn_tiled_fwd_f32_kernel, grid, dim3(TL_THREADS), 0, s, (const float*)qkv, (float*)o, lse, n, h, nblk);
    THEIA_CHECK_LAUNCH("theia_attention_fwd(tiled)");
    return THEIA_OK;
}

int theia_attention_bwd_tiled(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv, float* delta, int b, int n,
                              int h, int dtype, hipStream_t s) {
    const int rc = tl_check("theia_attention_bwd", b, n, h);
    if (rc != THEIA_OK) return rc;
    // dQ is written while other workgroups still read Q / K / V, delta while lse / O / dO are read
    const size_t es = dtype == THEIA_BF16 ? 2 : 4, nq = (size_t)b * n * h * 64 * es, nl = (size_t)b * n * h * sizeof(float);
    THEIA_CHECK_ARG(tl_disjoint(dqkv, 3 * nq, qkv, 3 * nq) && tl_disjoint(dqkv, 3 * nq, o, nq) && tl_disjoint(dqkv, 3 * nq, d_o, nq) &&
                        tl_disjoint(dqkv, 3 * nq, lse, nl) && tl_disjoint(dqkv, 3 * nq, delta, nl) && tl_disjoint(delta, nl, qkv, 3 * nq) &&
                        tl_disjoint(delta, nl, o, nq) && tl_disjoint(delta, nl, d_o, nq) && tl_disjoint(delta, nl, lse, nl),
                    "theia_attention_bwd(b=%d, n=%d, h=%d): dqkv / delta_ws overlap an input or each other", b, n, h);
    const int nblk = (n + TL_ROWS - 1) / TL_ROWS;
    const dim3 grid(b * h * nblk);
    const int64_t rows = (int64_t)b * n * h;
    const dim3 dgrid((unsigned)((rows + TL_THREADS / 8 - 1) / (TL_THREADS / 8)));
    if (dtype == THEIA_BF16) {
        hipLaunchKernelGGL(attn_tiled_delta_kernel<bf16_t>, dgrid, dim3(TL_THREADS), 0, s, (const bf16_t*)o, (const bf16_t*)d_o, delta, n, h, rows);
        THEIA_CHECK_LAUNCH("theia_attention_bwd(tiled delta)");
        hipLaunchKernelGGL(attn_tiled_dq_bf16_kernel, grid, dim3(TL_THREADS), 0, s, (const bf16_t*)qkv, (const bf16_t*)d_o, lse, delta,
                           (bf16_t*)dqkv, n, h, nblk);
        THEIA_CHECK_LAUNCH("theia_attention_bwd(tiled dq)");
        hipLaunchKernelGGL(attn_tiled_dkv_bf16_kernel, grid, dim3(TL_THREADS), 0, s, (const bf16_t*)qkv, (const bf16_t*)d_o, lse, delta,
                           (bf16_t*)dqkv, n, h, nblk);
    } else {
        hipLaunchKernelGGL(attn_tiled_delta_kernel<float>, dgrid, dim3(TL_THREADS), 0, s, (const float*)o, (const float*)d_o, delta, n, h, rows);
        THEIA_CHECK_LAUNCH("theia_attention_bwd(tiled delta)");
        hipLaunchKernelGGL(attn_tiled_dq_f32_kernel, grid, dim3(TL_THREADS), 0, s, (const float*)qkv, (const float*)d_o, lse, delta,
                           (float*)dqkv, n, h, nblk);
        THEIA_CHECK_LAUNCH("theia_attention_bwd(tiled dq)");
        hipLaunchKernelGGL(attn_tiled_dkv_f32_kernel, grid, dim3(TL_THREADS), 0, s, (const float*)qkv, (const float*)d_o, lse, delta,
                           (float*)dqkv, n, h, nblk);
    }
    THEIA_CHECK_LAUNCH("theia_attention_bwd(tiled dkv)");
    return THEIA_OK;
}
