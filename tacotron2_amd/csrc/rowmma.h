// The MFMA tile loop of the vocoders' products over a channel-last row image: out tile [128][BN] = A [128][K] B [BN][K]^T,
// once per precision family.  waveglow_layer.hip, hifigan.hip and vocos.hip call it from their own __global__ wrappers.
//
// 256 threads = 4 waves as WMW x WNW, a wave owns TM x TN MFMA tiles of 32 x 32 (BM = WMW TM 32 = 128, BN = WNW TN 32).
// B = weights [N][K], K contiguous, rows col0 .. col0 + BN - 1 (zero at and beyond N).  A is whatever the caller's `Rows`
// policy fetches; the loop knows neither taps nor halos nor the grid, so the wrapper reads blockIdx and the policy holds
//   RmStep step(int k0) const                      once per K-step (the tap of a tap-major K is a division);
//   float4 a(const RmStep& s, int r, int kc) const  columns kc .. kc + 3 of that step of tile row r (zero where the row
//                                                   does not exist);
//   void   epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const
// with acc[tm][tn] the 32 x 32 tile at tile rows (wm TM + tm) 32, columns (wn TN + tn) 32: column = lane & 31, row of
// element r = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
//
// Both bodies stage the next K-step in registers while the MFMAs run on the current LDS buffer (two buffers, one barrier a
// step).  Every output's sum runs over K in ascending order; within a K-step the split-bf16 products go al bh, ah bl, ah bh.
//   rm_tile_f32:  exact f32 on v_mfma_f32_32x32x2_f32, K-step 16, both operands transposed into k-major LDS (strides
//                 BM + 4 and BN + 4).
//   rm_tile_bf16: split-bf16 x 3 (X3) or plain bf16 on v_mfma_f32_32x32x16_bf16, K-step 32, K-contiguous bf16 LDS rows
//                 (stride 40), with the operand splitting of gemm.hip's bf16 kernels.
// K must be a multiple of 32 (the callers check their channel counts).
#pragma once
#include "common.h"

typedef short rm_bf16x8 __attribute__((ext_vector_type(8)));
#define RM_BK 16
#define RM_HK 32
#define RM_HLD 40

struct RmStep {
    int off, col;                       // the K-step's tap as a row offset, and its first column in that row
};

template <int TM, int TN>
__device__ __forceinline__ void rm_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

template <int WMW, int WNW, int TM, int TN, class Rows>
__device__ __forceinline__ void rm_tile_f32(const Rows& rows, const float* W, int N, int K, int col0) {
    constexpr int BM = WMW * TM * 32, BN = WNW * TN * 32;
    static_assert(BM == 128 && WMW * WNW == 4, "4 waves over 128 rows");
    constexpr int B_IT = (BN * 4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float As[2][RM_BK][BM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[2][RM_BK][BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WNW, wn = wave % WNW;
    const int nk = K / RM_BK;
    float4 ra[2], rb[B_IT];

    auto load = [&](int k0) {
        const RmStep s = rows.step(k0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + 256 * i;
            ra[i] = rows.a(s, f >> 2, (f & 3) * 4);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 2, kq = f & 3;
            const int gn = col0 + r;
            rb[i] = (f < BN * 4 && gn < N) ? *reinterpret_cast<const float4*>(W + (long long)gn * K + k0 + kq * 4)
                                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 2, kq = f & 3;
            As[buf][kq * 4 + 0][r] = ra[i].x;
            As[buf][kq * 4 + 1][r] = ra[i].y;
            As[buf][kq * 4 + 2][r] = ra[i].z;
            As[buf][kq * 4 + 3][r] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 2, kq = f & 3;
            if (f < BN * 4) {
                Bs[buf][kq * 4 + 0][r] = rb[i].x;
                Bs[buf][kq * 4 + 1][r] = rb[i].y;
                Bs[buf][kq * 4 + 2][r] = rb[i].z;
                Bs[buf][kq * 4 + 3][r] = rb[i].w;
            }
        }
    };

    f32x16 acc[TM][TN];
    rm_zero(acc);
    load(0);
    store(0);
    __syncthreads();
    const int l31 = lane & 31, lhi = lane >> 5;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) load((kt + 1) * RM_BK);
#pragma unroll
        for (int kk = 0; kk < RM_BK / 2; ++kk) {
            const int krow = kk * 2 + lhi;
            float a[TM], b[TN];
#pragma unroll
            for (int t = 0; t < TM; ++t) a[t] = As[cur][krow][(wm * TM + t) * 32 + l31];
#pragma unroll
            for (int t = 0; t < TN; ++t) b[t] = Bs[cur][krow][(wn * TN + t) * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    rows.epilogue(acc, wm, wn, lane);
}

template <bool X3, int WMW, int WNW, int TM, int TN, class Rows>
__device__ __forceinline__ void rm_tile_bf16(const Rows& rows, const float* W, int N, int K, int col0) {
    constexpr int NH = X3 ? 2 : 1;
    constexpr int BM = WMW * TM * 32, BN = WNW * TN * 32;
    static_assert(BM == 128 && WMW * WNW == 4, "4 waves over 128 rows");
    constexpr int B_IT = BN * 8 / 256;
    constexpr int IMGA = BM * RM_HLD, IMGB = BN * RM_HLD;
    __shared__ __attribute__((aligned(16))) unsigned short As[2][NH * IMGA];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[2][NH * IMGB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WNW, wn = wave % WNW;
    const int nk = K / RM_HK;
    float4 ra[4], rb[B_IT];

    auto load = [&](int k0) {
        const RmStep s = rows.step(k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = tid + 256 * i;
            ra[i] = rows.a(s, f >> 3, (f & 7) * 4);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 3, kq = f & 7;
            const int gn = col0 + r;
            rb[i] = gn < N ? *reinterpret_cast<const float4*>(W + (long long)gn * K + k0 + kq * 4)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // one float4 of a row to its bf16 image: the rounded halves, and under X3 the rounded remainders `img` shorts further on
    auto put = [&](unsigned short* S, int img, int f, const float4& v) {
        const int r = f >> 3, kq = f & 7;
        uint2 hi;
        hi.x = t2_cvt_pk_bf16(v.x, v.y);
        hi.y = t2_cvt_pk_bf16(v.z, v.w);
        *reinterpret_cast<uint2*>(&S[r * RM_HLD + kq * 4]) = hi;
        if (X3) {
            uint2 lo;
            lo.x = t2_cvt_pk_bf16(v.x - __uint_as_float(hi.x << 16), v.y - __uint_as_float(hi.x & 0xffff0000u));
            lo.y = t2_cvt_pk_bf16(v.z - __uint_as_float(hi.y << 16), v.w - __uint_as_float(hi.y & 0xffff0000u));
            *reinterpret_cast<uint2*>(&S[img + r * RM_HLD + kq * 4]) = lo;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) put(As[buf], IMGA, tid + 256 * i, ra[i]);
#pragma unroll
        for (int i = 0; i < B_IT; ++i) put(Bs[buf], IMGB, tid + 256 * i, rb[i]);
    };
    auto frag = [&](const unsigned short* S, int row, int ks, int lhi_) -> rm_bf16x8 {
        return *reinterpret_cast<const rm_bf16x8*>(&S[row * RM_HLD + ks * 16 + lhi_ * 8]);
    };

    f32x16 acc[TM][TN];
    rm_zero(acc);
    load(0);
    store(0);
    __syncthreads();
    const int l31 = lane & 31, lhi = lane >> 5;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) load((kt + 1) * RM_HK);
#pragma unroll
        for (int ks = 0; ks < RM_HK / 16; ++ks) {
            rm_bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                ah[t] = frag(As[cur], (wm * TM + t) * 32 + l31, ks, lhi);
                if (X3) al[t] = frag(As[cur] + IMGA, (wm * TM + t) * 32 + l31, ks, lhi);
            }
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                bh[t] = frag(Bs[cur], (wn * TN + t) * 32 + l31, ks, lhi);
                if (X3) bl[t] = frag(Bs[cur] + IMGB, (wn * TN + t) * 32 + l31, ks, lhi);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (X3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        if (more) store(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    rows.epilogue(acc, wm, wn, lane);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// precision 0 exact f32, 1 split-bf16 x 3, 2 bf16: the caller's three wrappers of one tile shape
template <class P>
static void rm_launch(int precision, void (*f32)(P), void (*bf16x3)(P), void (*bf16)(P), dim3 grid, hipStream_t s, const P& p) {
    T2_LAUNCH(precision == 0 ? f32 : (precision == 1 ? bf16x3 : bf16), grid, dim3(256), 0, s, p);
}

// The widest column tile that divides N (a multiple of 32), so that C = 32 and 64 still fill their MFMA tiles ...
static inline int rm_tile_cols(int N) { return N % 128 == 0 ? 128 : (N % 64 == 0 ? 64 : 32); }

// ... and its launch: F32K<WMW, WNW, TM, TN> and BF16K<X3, WMW, WNW, TM, TN> are the caller's wrappers.  128 columns are
// 2 x 2 waves of 2 x 2 tiles, 64 columns 2 x 2 waves of 2 x 1, 32 columns 4 x 1 waves of one tile.
#define RM_LAUNCH_SHAPE(F32K, BF16K, WMW, WNW, TM, TN, precision, grid, s, p)                                              \
    rm_launch(precision, F32K<WMW, WNW, TM, TN>, BF16K<true, WMW, WNW, TM, TN>, BF16K<false, WMW, WNW, TM, TN>, grid, s, p)
#define RM_LAUNCH_COLS(F32K, BF16K, BN, precision, grid, s, p)                                                             \
    do {                                                                                                                   \
        if ((BN) == 128)                                                                                                   \
            RM_LAUNCH_SHAPE(F32K, BF16K, 2, 2, 2, 2, precision, grid, s, p);                                               \
        else if ((BN) == 64)                                                                                               \
            RM_LAUNCH_SHAPE(F32K, BF16K, 2, 2, 2, 1, precision, grid, s, p);                                               \
        else                                                                                                               \
            RM_LAUNCH_SHAPE(F32K, BF16K, 4, 1, 1, 1, precision, grid, s, p);                                               \
    } while (0)
