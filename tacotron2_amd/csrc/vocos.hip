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
// vc_linear: out[m][n] = epi(bias[n] + sum_k X[m][k] W[n][k]) on 128 x BN tiles (BN = 128 / 64 / 32), the tile loop of
// csrc/rowmma.h that waveglow_layer.hip and hifigan.hip run too.  This file owns the parameters, how a row of A is fetched
// (VcRows: no taps), the epilogue, the __global__ wrappers with their grid mapping, and the C entry.  epi 0: v; 1: exact GELU v (1 + erf(v / sqrt 2)) / 2; 2: res[m][n] + gamma[n] v.
// Precision 0 exact f32 (v_mfma_f32_32x32x2_f32), 1 split-bf16 x 3, 2 bf16 (v_mfma_f32_32x32x16_bf16).  A row's sum runs over
// k in one fixed order whatever tile it lies in, so a ragged batch equals every utterance alone, bit for bit.
#include "rowmma.h"

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

// The rows of one 128 x BN tile for csrc/rowmma.h: no taps, `row0 + r < P` the only guard.
struct VcRows {
    const VcLinParams& p;
    long long row0;
    int col0;
    __device__ __forceinline__ RmStep step(int k0) const { return {0, k0}; }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        return row0 + r < p.P ? *reinterpret_cast<const float4*>(p.X + (row0 + r) * p.ldx + s.col + kc)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        vc_epilogue<TM, TN>(p, acc, row0, col0, wm, wn, lane);
    }
};

// blockIdx.x = row tile, blockIdx.y = column tile
template <int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void vc_lin_f32_kernel(VcLinParams p) {
    const VcRows rows{p, (long long)blockIdx.x * 128, (int)blockIdx.y * (WNW * TN * 32)};
    rm_tile_f32<WMW, WNW, TM, TN>(rows, p.W, p.N, p.K, rows.col0);
}

template <bool X3, int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void vc_lin_bf16_kernel(VcLinParams p) {
    const VcRows rows{p, (long long)blockIdx.x * 128, (int)blockIdx.y * (WNW * TN * 32)};
    rm_tile_bf16<X3, WMW, WNW, TM, TN>(rows, p.W, p.N, p.K, rows.col0);
}

#define VC_MAX_WIDTH 16416              /* K and N: n_fft up to 16384, its 2 F = n_fft + 2 values padded to 32 */

extern "C" int t2amd_vc_linear_f32(const float* X, long long x_floats, long long ldx, long long P, int K, const float* W,
                                   long long w_floats, const float* bias, int N, int epi, const float* gamma, const float* res,
                                   long long ldres, long long res_floats, float* out, long long ldout, long long out_floats,
                                   const int* rowb0, long long n_rowb, int precision, void* stream) {
    T2_REQUIRE(X && W && out && rowb0, "vc_linear: null operand");
    T2_REQUIRE(P > 0 && P <= T2_MAX_ROWS && n_rowb >= P, "vc_linear: the row map does not cover the rows (at most 2^31 - 256)");
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
    const int BN = rm_tile_cols(N);
    dim3 grid(t2_cdiv(P, 128), N / BN, 1);
    RM_LAUNCH_COLS(vc_lin_f32_kernel, vc_lin_bf16_kernel, BN, precision, grid, s, p);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
