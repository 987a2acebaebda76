// Vocos vocoder (Siuzdak 2023) on the MI355X: inference, mel -> waveform at the frame rate (tacotron2_amd/vocos.py).
//
// Layout.  The frame-rate packed row space of hifigan.hip as it is: channel-last row images X [P][C] f32, the utterances
// packed with H = 3 zero rows before, between and after them (rowb0[p] = utterance or -1, rowr0[p] = frame).  Three rows cover
// the 7-tap windows of embed and dwconv, and the n_fft - hop samples by which an utterance's last frame extends past it.
// Every kernel writes all P rows of its output and writes ZERO on rows whose rowb0 is negative.
//
// Launches of one call (vocos.py): pack the mels (t2amd_hg_pack_mel_f32), embed (t2amd_hg_conv_f32), LayerNorm (vc_dwln with
// zero taps); per ConvNeXt block vc_dwln (dwconv + LayerNorm), vc_linear GELU (pwconv1), vc_linear gamma / residual (pwconv2);
// then LayerNorm, vc_linear (head), vc_polar, vc_linear against the window-folded inverse-DFT basis, vc_ola.  The I-wide
// intermediate of a block goes through HBM (DESIGN section 12 says why).  The row kernels are in vocos_rows.hip.
//
// vc_linear: out[m][n] = epi(bias[n] + sum_k X[m][k] W[n][k]) on 128 x BN tiles (BN = 128 / 64 / 32), the operand handling of
// hifigan.hip copied with its taps removed.  epi 0: v; 1: exact GELU v (1 + erf(v / sqrt 2)) / 2; 2: res[m][n] + gamma[n] v.
// Precision 0 exact f32 (v_mfma_f32_32x32x2_f32), 1 split-bf16 x 3, 2 bf16 (v_mfma_f32_32x32x16_bf16).  A row's sum runs over
// k in one fixed order whatever tile it lies in, so a ragged batch equals every utterance alone, bit for bit.
#include "common.h"

struct VcLinParams {
    const float* X;
    long long ldx, P;
    const float* W;
    const float* bias;
    int N, K;
    int epi;
    const float* gamma;
    const float* res;
    long long ldres;
    float* out;
    long long ldout;
    const int* rowb0;
};

__device__ __forceinline__ float vc_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// acc[tm][tn]: the 32 x 32 tile at rows row0 + wm TM 32 + tm 32, columns col0 + wn TN 32 + tn 32 (col = lane & 31)
template <int TM, int TN>
__device__ __forceinline__ void vc_epilogue(const VcLinParams& p, f32x16 (&acc)[TM][TN], long long row0, int col0, int wm, int wn,
                                            int lane) {
    const int l31 = lane & 31, lhi = lane >> 5;
    unsigned real = 0;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long gm = row0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (gm < p.P && p.rowb0[gm] >= 0) real |= 1u << (tm * 16 + r);
        }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int gn = col0 + (wn * TN + tn) * 32 + l31;
        if (gn >= p.N) continue;
        const float b = p.bias ? p.bias[gn] : 0.f;
        const float g = p.epi == 2 ? p.gamma[gn] : 0.f;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long gm = row0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (gm >= p.P) continue;
                float* op = p.out + gm * p.ldout + gn;
                if (!((real >> (tm * 16 + r)) & 1u)) {
                    *op = 0.f;
                    continue;
                }
                float v = acc[tm][tn][r] + b;
                if (p.epi == 1) v = vc_gelu(v);
                if (p.epi == 2) v = fmaf(g, v, p.res[gm * p.ldres + gn]);
                *op = v;
            }
        }
    }
}

// ---- exact f32: 128 x BN x 16 tiles, both operands transposed into k-major LDS -----------------------------------------
#define VBK 16

template <int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void vc_lin_f32_kernel(VcLinParams p) {
    constexpr int BM = WMW * TM * 32, BN = WNW * TN * 32;
    static_assert(BM == 128 && WMW * WNW == 4, "4 waves over 128 rows");
    constexpr int B_IT = (BN * 4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float As[2][VBK][BM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[2][VBK][BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WNW, wn = wave % WNW;
    const long long row0 = (long long)blockIdx.x * BM;
    const int col0 = blockIdx.y * BN;
    const float* W = p.W;
    const int nk = p.K / VBK;
    float4 ra[2], rb[B_IT];

    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 2, kq = f & 3;
            ra[i] = row0 + r < p.P ? *reinterpret_cast<const float4*>(p.X + (row0 + r) * p.ldx + k0 + kq * 4)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 2, kq = f & 3;
            const int gn = col0 + r;
            rb[i] = (f < BN * 4 && gn < p.N) ? *reinterpret_cast<const float4*>(W + (long long)gn * p.K + k0 + kq * 4)
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
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load(0);
    store(0);
    __syncthreads();
    const int l31 = lane & 31, lhi = lane >> 5;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) load((kt + 1) * VBK);
#pragma unroll
        for (int kk = 0; kk < VBK / 2; ++kk) {
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
    vc_epilogue<TM, TN>(p, acc, row0, col0, wm, wn, lane);
}

// ---- split-bf16 x 3 (X3) / plain bf16: 128 x BN x 32 tiles, K-contiguous bf16 LDS rows (stride 40) --------------------
typedef short vc_bf16x8 __attribute__((ext_vector_type(8)));
#define VHK 32
#define VHLD 40

template <bool X3, int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void vc_lin_bf16_kernel(VcLinParams p) {
    constexpr int NH = X3 ? 2 : 1;
    constexpr int BM = WMW * TM * 32, BN = WNW * TN * 32;
    static_assert(BM == 128 && WMW * WNW == 4, "4 waves over 128 rows");
    constexpr int B_IT = BN * 8 / 256;
    constexpr int IMGA = BM * VHLD, IMGB = BN * VHLD;
    __shared__ __attribute__((aligned(16))) unsigned short As[2][NH * IMGA];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[2][NH * IMGB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WNW, wn = wave % WNW;
    const long long row0 = (long long)blockIdx.x * BM;
    const int col0 = blockIdx.y * BN;
    const float* W = p.W;
    const int nk = p.K / VHK;
    float4 ra[4], rb[B_IT];

    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 3, kq = f & 7;
            ra[i] = row0 + r < p.P ? *reinterpret_cast<const float4*>(p.X + (row0 + r) * p.ldx + k0 + kq * 4)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int f = tid + 256 * i;
            const int r = f >> 3, kq = f & 7;
            const int gn = col0 + r;
            rb[i] = gn < p.N ? *reinterpret_cast<const float4*>(W + (long long)gn * p.K + k0 + kq * 4)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto put = [&](unsigned short* S, int img, int f, const float4& v) {
        const int r = f >> 3, kq = f & 7;
        uint2 hi;
        hi.x = t2_cvt_pk_bf16(v.x, v.y);
        hi.y = t2_cvt_pk_bf16(v.z, v.w);
        *reinterpret_cast<uint2*>(&S[r * VHLD + kq * 4]) = hi;
        if (X3) {
            uint2 lo;
            lo.x = t2_cvt_pk_bf16(v.x - __uint_as_float(hi.x << 16), v.y - __uint_as_float(hi.x & 0xffff0000u));
            lo.y = t2_cvt_pk_bf16(v.z - __uint_as_float(hi.y << 16), v.w - __uint_as_float(hi.y & 0xffff0000u));
            *reinterpret_cast<uint2*>(&S[img + r * VHLD + kq * 4]) = lo;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) put(As[buf], IMGA, tid + 256 * i, ra[i]);
#pragma unroll
        for (int i = 0; i < B_IT; ++i) put(Bs[buf], IMGB, tid + 256 * i, rb[i]);
    };
    auto frag = [&](const unsigned short* S, int row, int ks, int lhi_) -> vc_bf16x8 {
        return *reinterpret_cast<const vc_bf16x8*>(&S[row * VHLD + ks * 16 + lhi_ * 8]);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load(0);
    store(0);
    __syncthreads();
    const int l31 = lane & 31, lhi = lane >> 5;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) load((kt + 1) * VHK);
#pragma unroll
        for (int ks = 0; ks < VHK / 16; ++ks) {
            vc_bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
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
    vc_epilogue<TM, TN>(p, acc, row0, col0, wm, wn, lane);
}

template <int WMW, int WNW, int TM, int TN>
static void vc_launch(const VcLinParams& p, int precision, dim3 grid, hipStream_t s) {
    if (precision == 0)
        T2_LAUNCH((vc_lin_f32_kernel<WMW, WNW, TM, TN>), grid, dim3(256), 0, s, p);
    else if (precision == 1)
        T2_LAUNCH((vc_lin_bf16_kernel<true, WMW, WNW, TM, TN>), grid, dim3(256), 0, s, p);
    else
        T2_LAUNCH((vc_lin_bf16_kernel<false, WMW, WNW, TM, TN>), grid, dim3(256), 0, s, p);
}

#define VC_MAX_ROWS 2147483392LL        /* 2^31 - 256 (grid.x = rows / 128) */
#define VC_MAX_WIDTH 16416              /* K and N: n_fft up to 16384, its 2 F = n_fft + 2 values padded to 32 */

extern "C" int t2amd_vc_linear_f32(const float* X, long long x_floats, long long ldx, long long P, int K, const float* W,
                                   long long w_floats, const float* bias, int N, int epi, const float* gamma, const float* res,
                                   long long ldres, long long res_floats, float* out, long long ldout, long long out_floats,
                                   const int* rowb0, long long n_rowb, int precision, void* stream) {
    T2_REQUIRE(X && W && out && rowb0, "vc_linear: null operand");
    T2_REQUIRE(P > 0 && P <= VC_MAX_ROWS && n_rowb >= P, "vc_linear: the row map does not cover the rows (at most 2^31 - 256)");
    T2_REQUIRE(K >= 32 && K % 32 == 0 && K <= VC_MAX_WIDTH, "vc_linear: K must be a multiple of 32, at most 16416");
    T2_REQUIRE(N >= 32 && N % 32 == 0 && N <= VC_MAX_WIDTH, "vc_linear: N must be a multiple of 32, at most 16416");
    T2_REQUIRE(precision >= 0 && precision <= 2, "vc_linear: precision must be 0 (exact f32), 1 (split-bf16 x3) or 2 (bf16)");
    T2_REQUIRE(epi >= 0 && epi <= 2, "vc_linear: epi must be 0 (bias), 1 (GELU) or 2 (gamma and residual)");
    T2_REQUIRE(epi != 2 || (gamma && res && bias), "vc_linear: epi 2 needs bias, gamma and res");
    T2_REQUIRE(ldx >= K && ldx % 4 == 0 && t2_aligned16(X) && t2_aligned16(W), "vc_linear: X / W must be 16-byte aligned rows");
    T2_REQUIRE(ldout >= N && (epi != 2 || ldres >= N), "vc_linear: out / res rows too short");
    T2_REQUIRE(X != out, "vc_linear: out must not be X");
    T2_REQUIRE(x_floats >= (P - 1) * ldx + K, "vc_linear: X is shorter than its rows");
    T2_REQUIRE(w_floats >= (long long)N * K, "vc_linear: W is shorter than [N][K]");
    T2_REQUIRE(out_floats >= (P - 1) * ldout + N, "vc_linear: out is shorter than its rows");
    T2_REQUIRE(epi != 2 || res_floats >= (P - 1) * ldres + N, "vc_linear: res is shorter than its rows");
    VcLinParams p;
    p.X = X; p.ldx = ldx; p.P = P; p.W = W; p.bias = bias; p.N = N; p.K = K; p.epi = epi; p.gamma = gamma;
    p.res = res; p.ldres = ldres; p.out = out; p.ldout = ldout; p.rowb0 = rowb0;
    hipStream_t s = (hipStream_t)stream;
    const int BN = N % 128 == 0 ? 128 : (N % 64 == 0 ? 64 : 32);
    dim3 grid(t2_cdiv(P, 128), N / BN, 1);
    if (BN == 128)
        vc_launch<2, 2, 2, 2>(p, precision, grid, s);
    else if (BN == 64)
        vc_launch<2, 2, 2, 1>(p, precision, grid, s);
    else
        vc_launch<4, 1, 1, 1>(p, precision, grid, s);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
