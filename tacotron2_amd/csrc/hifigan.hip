// HiFi-GAN generator (Kong, Kim, Bae 2020) on the MI355X: inference, mel -> waveform (tacotron2_amd/hifigan.py).
//
// Layout.  Every stage keeps WaveGlow's channel-last row image X [P][C] f32.  The frame-rate row space (stage 0) packs the
// utterances with H0 zero rows before, between and after them (rowb0[f] = utterance or -1, rowr0[f] = frame); the row space of
// a stage whose rows are S times as many is EXACTLY that space times S: packed row p belongs to frame-level row p / S.  So
// one small map serves every stage, the transposed convolution writes output row u * m + phase for every input row m (halo
// rows map to halo rows), and the halo of a stage is H0 * S rows, which the caller sizes to the widest half-window.
// Every kernel here writes all P rows of its output and writes ZERO on rows whose rowb0 is negative, so no buffer needs a
// memset and a halo row never holds "bias + neighbours"; operand rows outside [0, P) read as zero.
//
// hg_conv_*: out[u m + ph][n] = epi(bias[n] + sum_(tap, c) act(X[m + off(tap)][c]) W[ph][n][tap Cin + c]) on 128 x BN tiles
// (BN = 128 / 64 / 32, so C = 32 and 64 still fill their MFMA tiles), K tap-major as in waveglow_layer.hip.
//   convolution:            ph = 0, u = 1, off(tap) = (tap - (taps - 1) / 2) dil
//   transposed convolution: ph = blockIdx.z < u, q = ph + pad, off(tap) = q / u - tap, W[ph] the weight slice kk = q % u + u tap
// act = leaky-ReLU on the operand while it is loaded (leaky_relu(0) = 0, so zero halos stay zero).
// epi: v = acc + bias (+ res[row][n]);  v *= scale;  out = accumulate ? out + v : v  -- plain store, residual, and the
// multi-receptive-field sum (first block stores, later blocks add, one launch after the other: no atomics).
// Precision 0 exact f32 (v_mfma_f32_32x32x2_f32), 1 split-bf16 x 3, 2 bf16 (v_mfma_f32_32x32x16_bf16).
// The two element-wise ends of the path (mel packing, conv_post) are in hifigan_post.hip.
//
// The tile loop itself (LDS images, K loop, MFMA nest, once per precision family) is csrc/rowmma.h, shared with
// waveglow_layer.hip and vocos.hip.  This file owns the parameters, how a row of A is fetched (HgRows: bounds test,
// leaky-ReLU, the phase's taps), the epilogue, the __global__ wrappers with their grid mapping, and the C entries.
#include "rowmma.h"

struct HgConvParams {
    const float* X;
    long long ldx, P;
    const float* W;
    const float* bias;
    int N, K, Cin, taps;
    int tap_base, tap_step;       // convolution; the transposed form derives them from the phase
    int up, pad;
    int act;
    float slope;
    const float* res;
    long long ldres;
    float* out;
    long long ldout;
    float scale;
    int accumulate;
    const int* rowb0;
    int rdiv;
};

__device__ __forceinline__ float hg_lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }
__device__ __forceinline__ float4 hg_lrelu4(float4 v, float s) {
    return make_float4(hg_lrelu(v.x, s), hg_lrelu(v.y, s), hg_lrelu(v.z, s), hg_lrelu(v.w, s));
}

// acc[tm][tn]: the 32 x 32 tile at rows row0 + wm TM 32 + tm 32, columns col0 + wn TN 32 + tn 32 (col = lane & 31)
template <int TM, int TN>
__device__ __forceinline__ void hg_conv_epilogue(const HgConvParams& p, f32x16 (&acc)[TM][TN], long long row0, int col0, int wm,
                                                 int wn, int lane, int phase) {
    const int l31 = lane & 31, lhi = lane >> 5;
    unsigned real = 0;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long gm = row0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (gm < p.P && p.rowb0[gm / p.rdiv] >= 0) real |= 1u << (tm * 16 + r);
        }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int gn = col0 + (wn * TN + tn) * 32 + l31;
        if (gn >= p.N) continue;
        const float b = p.bias ? p.bias[gn] : 0.f;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long gm = row0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (gm >= p.P) continue;
                const long long orow = gm * p.up + phase;
                float* op = p.out + orow * p.ldout + gn;
                if (!((real >> (tm * 16 + r)) & 1u)) {
                    *op = 0.f;
                    continue;
                }
                float v = acc[tm][tn][r] + b;
                if (p.res) v += p.res[orow * p.ldres + gn];
                v *= p.scale;
                *op = p.accumulate ? *op + v : v;
            }
        }
    }
}

__device__ __forceinline__ void hg_taps(const HgConvParams& p, int phase, int& base, int& step) {
    if (p.up > 1) {
        base = (phase + p.pad) / p.up;
        step = -1;
    } else {
        base = p.tap_base;
        step = p.tap_step;
    }
}

// The rows of one 128 x BN tile for csrc/rowmma.h: 64-bit rows, every shifted row tested against [0, P), leaky-ReLU on the
// operand while it is loaded, the tap of a K-step taken once per step.  Build it in place in the kernel: returned by value
// from a helper, the reference it holds keeps the compiler from reading the kernel arguments once at entry, and the epilogue
// then re-reads them from memory row by row.
struct HgRows {
    const HgConvParams& p;
    long long row0;
    int col0, phase, tbase, tstep;
    __device__ __forceinline__ HgRows(const HgConvParams& p_, long long row0_, int col0_, int phase_)
        : p(p_), row0(row0_), col0(col0_), phase(phase_) {
        hg_taps(p, phase, tbase, tstep);
    }
    __device__ __forceinline__ RmStep step(int k0) const {
        const int tap = k0 / p.Cin;
        return {tbase + tap * tstep, k0 - tap * p.Cin};
    }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const long long src = row0 + r + s.off;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < p.P && src >= 0 && src < p.P) {
            v = *reinterpret_cast<const float4*>(p.X + src * p.ldx + s.col + kc);
            if (p.act) v = hg_lrelu4(v, p.slope);
        }
        return v;
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        hg_conv_epilogue<TM, TN>(p, acc, row0, col0, wm, wn, lane, phase);
    }
};

// blockIdx.x = row tile, blockIdx.y = column tile, blockIdx.z = phase (W[phase] the weight slice of a transposed convolution)
template <int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void hg_conv_f32_kernel(HgConvParams p) {
    const HgRows rows(p, (long long)blockIdx.x * 128, blockIdx.y * (WNW * TN * 32), blockIdx.z);
    rm_tile_f32<WMW, WNW, TM, TN>(rows, p.W + (long long)rows.phase * p.N * p.K, p.N, p.K, rows.col0);
}

template <bool X3, int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void hg_conv_bf16_kernel(HgConvParams p) {
    const HgRows rows(p, (long long)blockIdx.x * 128, blockIdx.y * (WNW * TN * 32), blockIdx.z);
    rm_tile_bf16<X3, WMW, WNW, TM, TN>(rows, p.W + (long long)rows.phase * p.N * p.K, p.N, p.K, rows.col0);
}

static int hg_conv_run(HgConvParams& p, long long x_floats, long long w_floats, long long res_floats, long long out_floats,
                       long long n_rowb, int precision, void* stream) {
    T2_REQUIRE(p.X && p.W && p.out && p.rowb0, "hg_conv: null operand");
    T2_REQUIRE(p.P > 0 && p.N > 0 && p.Cin > 0 && p.taps >= 1 && p.up >= 1, "hg_conv: bad dims");
    T2_REQUIRE(p.Cin % 32 == 0 && p.Cin <= 512, "hg_conv: input channels must be a multiple of 32, at most 512");
    T2_REQUIRE(p.N % 32 == 0 && p.N <= 512, "hg_conv: output channels must be a multiple of 32, at most 512");
    T2_REQUIRE(precision >= 0 && precision <= 2, "hg_conv: precision must be 0 (exact f32), 1 (split-bf16 x3) or 2 (bf16)");
    T2_REQUIRE(p.ldx >= p.Cin && p.ldx % 4 == 0 && t2_aligned16(p.X) && t2_aligned16(p.W),
               "hg_conv: X / W must be 16-byte aligned rows");
    T2_REQUIRE(p.ldout >= p.N && (!p.res || p.ldres >= p.N), "hg_conv: out / res rows too short");
    T2_REQUIRE(p.rdiv >= 1 && p.P % p.rdiv == 0 && n_rowb >= p.P / p.rdiv, "hg_conv: the row map does not cover the rows");
    T2_REQUIRE(p.P * p.up <= T2_MAX_ROWS, "hg_conv: too many rows");
    T2_REQUIRE(x_floats >= (p.P - 1) * p.ldx + p.Cin, "hg_conv: X is shorter than its rows");
    T2_REQUIRE(w_floats >= (long long)p.up * p.N * p.K, "hg_conv: W is shorter than [phases][N][taps Cin]");
    T2_REQUIRE(out_floats >= (p.P * p.up - 1) * p.ldout + p.N, "hg_conv: out is shorter than its rows");
    T2_REQUIRE(!p.res || res_floats >= (p.P * p.up - 1) * p.ldres + p.N, "hg_conv: res is shorter than its rows");
    hipStream_t s = (hipStream_t)stream;
    const int BN = rm_tile_cols(p.N);
    dim3 grid(t2_cdiv(p.P, 128), p.N / BN, p.up);
    RM_LAUNCH_COLS(hg_conv_f32_kernel, hg_conv_bf16_kernel, BN, precision, grid, s, p);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_hg_conv_f32(const float* X, long long x_floats, long long ldx, long long P, int Cin, const float* W,
                                 long long w_floats, const float* bias, int N, int taps, int dil, int act, float slope,
                                 const float* res, long long ldres, long long res_floats, float* out, long long ldout,
                                 long long out_floats, float scale, int accumulate, const int* rowb0, long long n_rowb, int rdiv,
                                 int precision, void* stream) {
    T2_REQUIRE(taps >= 1 && taps % 2 == 1, "hg_conv: the kernel size must be odd");
    T2_REQUIRE(dil >= 1 && (long long)dil * (taps - 1) / 2 < (1 << 20), "hg_conv: bad dilation");
    HgConvParams p;
    p.X = X; p.ldx = ldx; p.P = P; p.W = W; p.bias = bias;
    p.N = N; p.Cin = Cin; p.taps = taps; p.K = taps * Cin;
    p.tap_base = -((taps - 1) / 2) * dil; p.tap_step = dil; p.up = 1; p.pad = 0;
    p.act = act; p.slope = slope; p.res = res; p.ldres = ldres; p.out = out; p.ldout = ldout;
    p.scale = scale; p.accumulate = accumulate; p.rowb0 = rowb0; p.rdiv = rdiv;
    return hg_conv_run(p, x_floats, w_floats, res_floats, out_floats, n_rowb, precision, stream);
}

extern "C" int t2amd_hg_upsample_f32(const float* X, long long x_floats, long long ldx, long long P, int Cin, const float* W,
                                     long long w_floats, const float* bias, int N, int ku, int u, int act, float slope,
                                     float* out, long long ldout, long long out_floats, const int* rowb0, long long n_rowb,
                                     int rdiv, int precision, void* stream) {
    T2_REQUIRE(u >= 1 && u <= 64 && ku >= u && ku % u == 0, "hg_upsample: the kernel must be a multiple of the stride (at most 64)");
    T2_REQUIRE((ku - u) % 2 == 0, "hg_upsample: kernel - stride must be even");
    HgConvParams p;
    p.X = X; p.ldx = ldx; p.P = P; p.W = W; p.bias = bias;
    p.N = N; p.Cin = Cin; p.taps = ku / u; p.K = p.taps * Cin;
    p.up = u; p.pad = (ku - u) / 2;
    p.tap_base = p.pad / u; p.tap_step = -1;          // what hg_taps gives phase 0; the only phase when u = 1
    p.act = act; p.slope = slope; p.res = nullptr; p.ldres = 0; p.out = out; p.ldout = ldout;
    p.scale = 1.0f; p.accumulate = 0; p.rowb0 = rowb0; p.rdiv = rdiv;
    return hg_conv_run(p, x_floats, w_floats, 0, out_floats, n_rowb, precision, stream);
}
