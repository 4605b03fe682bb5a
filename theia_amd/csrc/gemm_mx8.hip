// OCP MX fp8 (MXFP8, e4m3 elements + E8M0 block scales) GEMM operands and the block-scaled NT GEMM of precision="mxfp8".
//
// Format (include/theia_hip.h, theia_quantize_mx8): blocks of 32 consecutive elements along K inside one row; per block
// amax = max |x|, e = clamp(floor(log2 amax) - 8, -127, 127), scale byte e + 127, q = e4m3(RNE(clamp(x * 2^-e, +-448)));
// an all-zero block stores scale byte 127 and 32 zero bytes.  Elements [rows][K] (packed), scales [rows][K/32].
//
//   quantize_mx8_kernel    4 lanes per block, 8 elements per lane (16-byte bf16 / 2 x 16-byte f32 loads), block max over the
//                          4 lanes by two xor shuffles: one pass, no atomics, deterministic.
//   gemm_nt_mx8_kernel     out[m,n] = epi( sum_k A[m,k] W[n,k] ) on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, f32
//                          accumulate).  128x128 tile, 4 waves of 64x64, K-steps of 128 bytes staged by LDS-DMA
//                          (global_load_lds_dwordx4) into two [rows][128 B] stages with the 16-byte chunk XOR-swizzled by
//                          (row>>1)&7 on the source side (the layout of the 2-stage kernel in gemm.hip).
// MFMA lane map (16x16x128 with 8-bit operands, measured on the GPU with one-hot data and a distinct scale per (row, block); pinned
// by the exact-integer test of tests/test_mx8_gpu.py): lane l (g = l>>4) holds row l&15, K bytes 16g .. 16g+15 in its first four
// VGPRs and 64+16g .. 64+16g+15 in the last four; the E8M0 scale of K block j (bytes 32j .. 32j+31) of row r comes from byte 0
// (op_sel 0) of the scale register of lane 16j + r.  So a lane reads 16-byte chunks g and 4+g of its row and supplies the scale of
// block g -- NOT the scale of the 32 bytes it holds (the obvious map, 32 consecutive bytes per lane, puts half of every block under
// the wrong scale).  The weight fragment is the MFMA A operand, the activation fragment the B operand, so the accumulators have
// the layout gt_epilogue (gemm_tile.h) takes: the epilogue, its arithmetic and its rounding are the bf16 theia_gemm_nt ones.
// Scales are read per K-step straight into registers (one byte per fragment and lane); the loads retire behind the same
// vmcnt(0) that closes every K-step.  Out-of-range rows, K chunks past K and scale blocks past K/32 read a page of zeros.
#include "gemm_tile.h"

typedef __attribute__((ext_vector_type(8))) int mx8_v8i;

__device__ uint4 g_mx8_zero[16];  // 256 B of zeros: source of out-of-range operand chunks and scale bytes

// ================================================================================================
// quantisation
// ================================================================================================
__device__ __forceinline__ void mx8_load8(const bf16_t* p, float (&v)[8]) { load8(p, v); }
__device__ __forceinline__ void mx8_load8(const float* p, float (&v)[8]) { load8(p, v); }

// quant block qb (row qb / nb, block qb % nb) of one tensor; sub = this lane's quarter of the block (8 elements)
template <typename T>
__device__ __forceinline__ void mx8_quant_block(const T* __restrict__ src, int64_t ld, int nb, int64_t qb, int sub, bool live,
                                                uint8_t* __restrict__ dst, uint8_t* __restrict__ dsc) {
    const int64_t row = live ? qb / nb : 0;
    const int blk = live ? (int)(qb - row * nb) : 0;
    const int K = nb * 32;
    float v[8];
    mx8_load8(src + row * ld + blk * 32 + sub * 8, v);
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(v[j]));
    am = fmaxf(am, __shfl_xor(am, 1));
    am = fmaxf(am, __shfl_xor(am, 2));
    // floor(log2 amax) from v_frexp_exp (amax = f * 2^x, f in [0.5, 1): x - 1), subnormal maxima included
    const int e = am == 0.f ? 0 : min(max(__builtin_amdgcn_frexp_expf(am) - 1 - 8, -127), 127);
    uint32_t lo = 0, hi = 0;
    if (am != 0.f) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = fminf(fmaxf(ldexpf(v[j], -e), -448.f), 448.f);  // exact: a power-of-two scaling
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
    }
    if (live) {
        *reinterpret_cast<uint2*>(dst + row * K + blk * 32 + sub * 8) = make_uint2(lo, hi);
        if (sub == 0) dsc[row * nb + blk] = (uint8_t)(e + 127);
    }
}

// 64 quant blocks per 256-thread workgroup
template <typename T>
__global__ __launch_bounds__(256) void quantize_mx8_kernel(const T* __restrict__ src, int64_t rows, int nb, int64_t ld,
                                                           uint8_t* __restrict__ dst, uint8_t* __restrict__ dsc) {
    const int64_t qb = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    const bool live = qb < rows * nb;  // (dead lanes still take part in the shuffles, on row 0)
    mx8_quant_block<T>(src, ld, nb, qb, threadIdx.x & 3, live, dst, dsc);
}

__global__ __launch_bounds__(256) void quantize_mx8_batch_kernel(const theia_mx8_job_t* __restrict__ jobs, int njobs) {
    const int64_t b = blockIdx.x;
    int lo = 0, hi = njobs - 1;  // last job with first_block <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= b) lo = mid;
        else hi = mid - 1;
    }
    const theia_mx8_job_t& j = jobs[lo];
    const int nb = j.K / 32;
    const int64_t qb = (b - j.first_block) * 64 + (threadIdx.x >> 2);
    const bool live = qb < j.rows * nb;
    if (j.src_dtype == THEIA_F32)
        mx8_quant_block<float>(reinterpret_cast<const float*>(j.src), j.ld, nb, qb, threadIdx.x & 3, live, j.dst, j.dst_scale);
    else
        mx8_quant_block<bf16_t>(reinterpret_cast<const bf16_t*>(j.src), j.ld, nb, qb, threadIdx.x & 3, live, j.dst, j.dst_scale);
}

static int mx8_check_quant(const char* who, const void* src, int src_dtype, int64_t rows, int K, int64_t ld, const uint8_t* dst,
                           const uint8_t* dsc) {
    THEIA_CHECK_ARG(src != nullptr && dst != nullptr && dsc != nullptr, "%s: null pointer", who);
    THEIA_CHECK_ARG(src_dtype == THEIA_F32 || src_dtype == THEIA_BF16, "%s: src_dtype %d (THEIA_F32 / THEIA_BF16)", who, src_dtype);
    THEIA_CHECK_ARG(rows >= 1 && rows < ((int64_t)1 << 40), "%s: rows=%lld", who, (long long)rows);
    THEIA_CHECK_ARG(K >= 32 && K % 32 == 0, "%s: K=%d must be a positive multiple of 32", who, K);
    THEIA_CHECK_ARG(ld >= K, "%s: ld=%lld < K=%d", who, (long long)ld, K);
    const int esz = src_dtype == THEIA_F32 ? 4 : 2;
    THEIA_CHECK_ARG((ld * esz) % 16 == 0 && (uintptr_t)src % 16 == 0, "%s: the source rows must be 16-byte aligned", who);
    THEIA_CHECK_ARG((uintptr_t)dst % 8 == 0, "%s: dst must be 8-byte aligned", who);
    return THEIA_OK;
}

extern "C" int theia_quantize_mx8(const void* src, int src_dtype, int64_t rows, int K, int64_t ld, uint8_t* dst, uint8_t* dst_scale,
                                  void* stream) {
    const int rc = mx8_check_quant("theia_quantize_mx8", src, src_dtype, rows, K, ld, dst, dst_scale);
    if (rc != THEIA_OK) return rc;
    const int nb = K / 32;
    const int64_t grid = (rows * nb + 63) / 64;
    THEIA_CHECK_ARG(grid < ((int64_t)1 << 31), "theia_quantize_mx8: too many blocks");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (src_dtype == THEIA_F32)
        hipLaunchKernelGGL(quantize_mx8_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, (const float*)src, rows, nb, ld, dst, dst_scale);
    else
        hipLaunchKernelGGL(quantize_mx8_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)src, rows, nb, ld, dst, dst_scale);
    THEIA_CHECK_LAUNCH("theia_quantize_mx8");
    return THEIA_OK;
}

extern "C" int64_t theia_quantize_mx8_batch_plan(theia_mx8_job_t* jobs, int njobs) {
    if (jobs == nullptr || njobs < 1) {
        theia_set_error("theia_quantize_mx8_batch_plan: empty table");
        return THEIA_ERR_INVALID;
    }
    int64_t total = 0;
    for (int i = 0; i < njobs; ++i) {
        const theia_mx8_job_t& j = jobs[i];
        const int rc = mx8_check_quant("theia_quantize_mx8_batch_plan", j.src, j.src_dtype, j.rows, j.K, j.ld, j.dst, j.dst_scale);
        if (rc != THEIA_OK) return rc;
        jobs[i].first_block = total;
        total += (j.rows * (j.K / 32) + 63) / 64;
    }
    if (total >= ((int64_t)1 << 31)) {
        theia_set_error("theia_quantize_mx8_batch_plan: too many blocks");
        return THEIA_ERR_INVALID;
    }
    return total;
}

extern "C" int theia_quantize_mx8_batch(const theia_mx8_job_t* jobs_device, int njobs, int64_t total_blocks, void* stream) {
    THEIA_CHECK_ARG(jobs_device != nullptr && njobs >= 1, "theia_quantize_mx8_batch: empty table");
    THEIA_CHECK_ARG(total_blocks >= 1 && total_blocks < ((int64_t)1 << 31), "theia_quantize_mx8_batch: total_blocks=%lld",
                    (long long)total_blocks);
    hipLaunchKernelGGL(quantize_mx8_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       jobs_device, njobs);
    THEIA_CHECK_LAUNCH("theia_quantize_mx8_batch");
    return THEIA_OK;
}

// ================================================================================================
// block-scaled NT GEMM
// ================================================================================================
namespace {
constexpr int MX_BM = 128, MX_BN = 128, MX_WM = 64, MX_WN = 64;
constexpr int MX_FM = MX_WM / 16, MX_FN = MX_WN / 16;
constexpr int MX_SRP = 32;                          // rows staged per pass (256 threads x 16 B = 32 rows of 128 B)
constexpr int MX_NPA = MX_BM / MX_SRP, MX_NPB = MX_BN / MX_SRP;
constexpr int MX_STAGE = (MX_BM + MX_BN) * 128;     // bytes per K-step stage
constexpr int MX_EP_BYTES = 4 * MX_WM * (MX_WN + 4) * 4;
constexpr int MX_LDS = 2 * MX_STAGE > MX_EP_BYTES ? 2 * MX_STAGE : MX_EP_BYTES;
}  // namespace

__device__ __forceinline__ mx8_v8i mx8_join(const gt_u32x4& lo, const gt_u32x4& hi) {
    return __builtin_bit_cast(mx8_v8i, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// global_load_ubyte with no compiler-inserted wait (see load_scales below).  CONSTRAINT: the compiler believes the destination is
// written when this statement issues, so nothing may read it before the s_waitcnt vmcnt(0) of mx8_wait_vm, which names every such
// register as an in/out operand: the values are only ever used after that statement.  Every use of the loaded scales must go through
// mx8_wait_vm first (the kernel copies sca_n / scw_n into sca / scw only after it), and the loads must not sit in a branch whose
// results are merged (see the K loop); the exact-integer GEMM test covers K up to 3072.
__device__ __forceinline__ int mx8_load_u8(uint64_t addr) {
    int v;
    asm volatile("global_load_ubyte %0, %1, off" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ void mx8_wait_vm(int (&a)[MX_FM], int (&w)[MX_FN]) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3])::"memory");
}

__global__ __launch_bounds__(256, 2) void gemm_nt_mx8_kernel(const theia_gemm_mx8_args_t p, const theia_gemm_args_t e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (p.N + MX_BN - 1) / MX_BN;
    const int tile = gt_xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (tile / tiles_n) * MX_BM, n0 = (tile % tiles_n) * MX_BN;
    const int nb = p.K / 32;
    const uint64_t zp = reinterpret_cast<uint64_t>(g_mx8_zero);

    // ---- staging rows of this thread (fixed for the whole K loop) ----
    const int st_chunk = tid & 7, st_row = tid >> 3;
    const int lchunk = st_chunk ^ ((st_row >> 1) & 7);
    uint64_t a_src[MX_NPA], w_src[MX_NPB];
    bool a_ok[MX_NPA], w_ok[MX_NPB];
#pragma unroll
    for (int i = 0; i < MX_NPA; ++i) {
        const int m = m0 + st_row + MX_SRP * i;
        a_ok[i] = m < p.M;
        a_src[i] = reinterpret_cast<uint64_t>(p.a + (int64_t)(a_ok[i] ? m : 0) * p.lda + lchunk * 16);
    }
#pragma unroll
    for (int i = 0; i < MX_NPB; ++i) {
        const int n = n0 + st_row + MX_SRP * i;
        w_ok[i] = n < p.N;
        w_src[i] = reinterpret_cast<uint64_t>(p.w + (int64_t)(w_ok[i] ? n : 0) * p.ldw + lchunk * 16);
    }
    // ---- scale rows of this lane's fragments: lane l supplies block (l >> 4) of the K-step for row l & 15 ----
    const int frow = lane & 15, fg = lane >> 4;
    uint64_t as_row[MX_FM], ws_row[MX_FN];
    bool as_ok[MX_FM], ws_ok[MX_FN];
#pragma unroll
    for (int j = 0; j < MX_FM; ++j) {
        const int m = m0 + wm * MX_WM + j * 16 + frow;
        as_ok[j] = m < p.M;
        as_row[j] = reinterpret_cast<uint64_t>(p.a_scale + (int64_t)(as_ok[j] ? m : 0) * nb + fg);
    }
#pragma unroll
    for (int i = 0; i < MX_FN; ++i) {
        const int n = n0 + wn * MX_WN + i * 16 + frow;
        ws_ok[i] = n < p.N;
        ws_row[i] = reinterpret_cast<uint64_t>(p.w_scale + (int64_t)(ws_ok[i] ? n : 0) * nb + fg);
    }

    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    // K-step kt -> stage `stage`: 4 + 4 LDS-DMA pieces per thread (branch-free: the source address is selected with masks)
    auto issue_tile = [&](int kt, int stage) {
        const int c = kt * 128;
        const bool cok = c + lchunk * 16 < p.K;
        char* sa = smem + stage * MX_STAGE + uwave * (8 * 128);
        char* sb = sa + MX_BM * 128;
#pragma unroll
        for (int i = 0; i < MX_NPA + MX_NPB; ++i) {
            const bool ok = cok & (i < MX_NPA ? a_ok[i] : w_ok[i - MX_NPA]);
            const uint64_t msk = 0ull - (uint64_t)ok;
            const uint64_t src = ((i < MX_NPA ? a_src[i] : w_src[i - MX_NPA]) + c) & msk | (zp & ~msk);
            char* dst = i < MX_NPA ? sa + i * (MX_SRP * 128) : sb + (i - MX_NPA) * (MX_SRP * 128);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
    };
    // scale bytes of K-step kt (one per fragment), loaded by inline asm: invisible to the compiler's vmcnt bookkeeping (as the
    // LDS-DMA pieces are), so it does not wait for them -- and with them for the whole prefetch -- before the MFMAs of this K-step;
    // mx8_wait_vm ties the registers to the wait that retires them
    auto load_scales = [&](int kt, int (&sa)[MX_FM], int (&sw)[MX_FN]) {
        const int blk = kt * 4;
        const bool bok = blk + fg < nb;
#pragma unroll
        for (int j = 0; j < MX_FM; ++j) {
            const uint64_t msk = 0ull - (uint64_t)(bok & as_ok[j]);
            sa[j] = mx8_load_u8(((as_row[j] + blk) & msk) | (zp & ~msk));
        }
#pragma unroll
        for (int i = 0; i < MX_FN; ++i) {
            const uint64_t msk = 0ull - (uint64_t)(bok & ws_ok[i]);
            sw[i] = mx8_load_u8(((ws_row[i] + blk) & msk) | (zp & ~msk));
        }
    };

    gt_f32x4 acc[MX_FN][MX_FM];
#pragma unroll
    for (int i = 0; i < MX_FN; ++i)
#pragma unroll
        for (int j = 0; j < MX_FM; ++j) acc[i][j] = (gt_f32x4){0.f, 0.f, 0.f, 0.f};

    const int nkt = (p.K + 127) / 128;
    int sca[MX_FM], scw[MX_FN];
    issue_tile(0, 0);
    load_scales(0, sca, scw);
    mx8_wait_vm(sca, scw);
    __syncthreads();

    // fragment addresses: row frow of the fragment, the 16-byte K chunks fg and 4 + fg (swizzled by (row >> 1) & 7, row = 16*f + frow)
    const int sw = (frow >> 1) & 7;
    const uint32_t lds0 = gt_lds_addr(smem);
    const uint32_t ra0 = lds0 + (wm * MX_WM + frow) * 128 + ((fg ^ sw) << 4);
    const uint32_t ra1 = lds0 + (wm * MX_WM + frow) * 128 + (((4 + fg) ^ sw) << 4);
    const uint32_t rb0 = lds0 + MX_BM * 128 + (wn * MX_WN + frow) * 128 + ((fg ^ sw) << 4);
    const uint32_t rb1 = lds0 + MX_BM * 128 + (wn * MX_WN + frow) * 128 + (((4 + fg) ^ sw) << 4);

    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        // the last step re-fetches its own tile into the idle stage instead of branching around the prefetch: with the scale loads
        // inside a branch the compiler merges their results with the other path's values right after the (asm) loads, i.e. before the
        // wait, and the MFMAs read stale scale registers (NaN outputs at K = 3072 when tried)
        const int ktn = min(kt + 1, nkt - 1);
        issue_tile(ktn, cur ^ 1);
        int sca_n[MX_FM], scw_n[MX_FN];
        load_scales(ktn, sca_n, scw_n);

        const uint32_t so = cur * MX_STAGE;
        gt_u32x4 fa[2 * MX_FM], fw[2 * MX_FN];  // [2f] = chunk fg, [2f+1] = chunk 4+fg
        gt_ds_read128<0 * 2048>(fw[0], rb0 + so);
        gt_ds_read128<0 * 2048>(fw[1], rb1 + so);
        gt_ds_read128<1 * 2048>(fw[2], rb0 + so);
        gt_ds_read128<1 * 2048>(fw[3], rb1 + so);
        gt_ds_read128<2 * 2048>(fw[4], rb0 + so);
        gt_ds_read128<2 * 2048>(fw[5], rb1 + so);
        gt_ds_read128<3 * 2048>(fw[6], rb0 + so);
        gt_ds_read128<3 * 2048>(fw[7], rb1 + so);
        gt_ds_read128<0 * 2048>(fa[0], ra0 + so);
        gt_ds_read128<0 * 2048>(fa[1], ra1 + so);
        gt_ds_read128<1 * 2048>(fa[2], ra0 + so);
        gt_ds_read128<1 * 2048>(fa[3], ra1 + so);
        gt_ds_read128<2 * 2048>(fa[4], ra0 + so);
        gt_ds_read128<2 * 2048>(fa[5], ra1 + so);
        gt_ds_read128<3 * 2048>(fa[6], ra0 + so);
        gt_ds_read128<3 * 2048>(fa[7], ra1 + so);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(fw[0]), "+v"(fw[1]), "+v"(fw[2]), "+v"(fw[3]), "+v"(fw[4]), "+v"(fw[5]), "+v"(fw[6]), "+v"(fw[7]),
                       "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fa[4]), "+v"(fa[5]), "+v"(fa[6]), "+v"(fa[7])::"memory");
#pragma unroll
        for (int j = 0; j < MX_FM; ++j) {
            const mx8_v8i b = mx8_join(fa[2 * j], fa[2 * j + 1]);
#pragma unroll
            for (int i = 0; i < MX_FN; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mx8_join(fw[2 * i], fw[2 * i + 1]), b, acc[i][j], 0, 0, 0,
                                                                              scw[i], 0, sca[j]);
        }
        // keep the MFMAs above the wait (they do not depend on it, and the scheduler would otherwise sink them below it and expose
        // the whole prefetch latency); then K-step kt+1 (tiles and scales) has landed
        __builtin_amdgcn_sched_barrier(0);
        mx8_wait_vm(sca_n, scw_n);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MX_FM; ++j) sca[j] = sca_n[j];
#pragma unroll
        for (int i = 0; i < MX_FN; ++i) scw[i] = scw_n[i];
    }
    // ---- epilogue of the bf16 GEMM (gemm_tile.h): wave-private LDS round trip, 16-byte vector global accesses ----
    float* ep = reinterpret_cast<float*>(smem) + wave * (MX_WM * (MX_WN + 4));
    gt_epilogue<bf16_t, MX_WM, MX_WN>(acc, ep, e, m0 + wm * MX_WM, n0 + wn * MX_WN, lane);
}

extern "C" int theia_gemm_nt_mx8(const theia_gemm_mx8_args_t* a, void* stream) {
    const char* who = "theia_gemm_nt_mx8";
    THEIA_CHECK_ARG(a != nullptr, "%s: null args", who);
    THEIA_CHECK_ARG(a->a != nullptr && a->a_scale != nullptr && a->w != nullptr && a->w_scale != nullptr && a->out != nullptr,
                    "%s: null operand / scale / output pointer", who);
    THEIA_CHECK_ARG(a->M >= 1 && a->M < (1 << 24), "%s: M=%d outside [1, 2^24)", who, a->M);
    THEIA_CHECK_ARG(a->N >= 8 && a->N % 8 == 0, "%s: N=%d must be a positive multiple of 8", who, a->N);
    THEIA_CHECK_ARG(a->K >= 32 && a->K % 32 == 0, "%s: K=%d must be a positive multiple of 32", who, a->K);
    THEIA_CHECK_ARG(a->lda >= a->K && a->ldw >= a->K && a->lda % 16 == 0 && a->ldw % 16 == 0,
                    "%s: lda=%d / ldw=%d must be >= K and multiples of 16", who, a->lda, a->ldw);
    THEIA_CHECK_ARG(a->ldo >= a->N && a->ldo % 8 == 0, "%s: ldo=%d must be >= N and a multiple of 8", who, a->ldo);
    THEIA_CHECK_ARG(((uintptr_t)a->a | (uintptr_t)a->w | (uintptr_t)a->out | (uintptr_t)a->bias | (uintptr_t)a->resid |
                     (uintptr_t)a->aux_in | (uintptr_t)a->aux_out) % 16 == 0,
                    "%s: operands, output, bias, resid and aux tensors must be 16-byte aligned", who);
    THEIA_CHECK_ARG(a->act >= THEIA_ACT_NONE && a->act <= THEIA_ACT_MUL_DRELU, "%s: act=%d", who, a->act);
    const bool mul = a->act == THEIA_ACT_MUL_DGELU || a->act == THEIA_ACT_MUL_DRELU;
    THEIA_CHECK_ARG(!mul || a->aux_in != nullptr, "%s: act %d needs aux_in", who, a->act);
    THEIA_CHECK_ARG(a->aux_out == nullptr || a->act == THEIA_ACT_GELU, "%s: aux_out is the GELU pre-activation (act GELU only)", who);

    // the epilogue's view of the launch: a plain row map, bf16 output (what theia_gemm_nt sees for ops.linear)
    theia_gemm_args_t e;
    memset(&e, 0, sizeof(e));
    e.out = a->out;
    e.bias = a->bias;
    e.resid = a->resid;
    e.aux_in = a->aux_in;
    e.aux_out = a->aux_out;
    e.M = a->M;
    e.N = a->N;
    e.K = a->K;
    e.ldw = a->ldw;
    e.ldo = a->ldo;
    e.act = a->act;
    e.map.ntaps = 1;
    e.map.rows_h = e.map.rows_w = e.map.in_h = e.map.in_w = 1;
    e.map.in_sy = e.map.in_sx = 1;
    e.map.in_c = a->K;
    e.map.out_w = 1;
    e.map.out_sy = e.map.out_sx = 1;
    e.map.in_batch_stride = a->lda;
    e.map.out_batch_stride = a->ldo;

    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_mx8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MX_LDS);
        attr_set = true;
    }
    const int64_t tiles = (int64_t)cdiv_i(a->M, MX_BM) * cdiv_i(a->N, MX_BN);
    hipLaunchKernelGGL(gemm_nt_mx8_kernel, dim3((unsigned)tiles), dim3(256), MX_LDS, reinterpret_cast<hipStream_t>(stream), *a, e);
    THEIA_CHECK_LAUNCH(who);
    return THEIA_OK;
}
