// WaveGlow WN layer products on the MFMA (see waveglow.hip for the layout and the rest of the inference path).
//
// The tile loop itself (LDS images, K loop, MFMA nest, once per precision family) is csrc/rowmma.h, shared with hifigan.hip
// and vocos.hip.  This file owns the parameters, how a row of A is fetched (WgRows), the three epilogues, the __global__
// wrappers with their grid mapping, and the C entries with their checks.
//
// Always 128 x 128 output tiles of 4 waves (2 x 2, 64 x 64 per wave = 2 x 2 MFMA tiles of 32 x 32; columns at and beyond N
// are masked), A = the channel-last row image, B = weights [N][K] (K contiguous).  K is tap-major: column tap * Cin + c of
// row m reads X[(m + (tap - (taps - 1) / 2) * dil) * ldx + c].  The caller points X at the first computed row of an image
// whose zero halo is at least dil rows deep on both sides, so no tap needs a bounds test and none crosses an utterance.
//
// mode 0 (gated in-layer product, N = 2C, K = 3C): the weight rows are packed so that column block 64 q + 0..31 holds the
// tanh channels 32 q .. 32 q + 31 and block 64 q + 32..63 their sigmoid partners.  A wave owns the 64 columns of one q,
// and the 32x32 MFMA puts the column on the lane (col = lane & 31), so both partners of a channel sit in the same lane:
//   acts[m][c] = tanh(acc_t + bias_t + cnd[m][c]) * sigmoid(acc_s + bias_s + cnd[m][C + c])
// The 2C-wide pre-activation never leaves registers.
// mode 1 (residual / skip product, K = C): column n < nres is added into h (rows whose rowb >= 0 only, so halo rows stay
// zero); column n >= nres goes to skip[m][n - nres] (stored when skip_store, else added).
//
// mode 2 (the in-layer product's data gradient, N = C, K = 3 * 2C over the image of d_pre, W = the transposed weights with
// the taps mirrored): column n is added into h[m][n] (stored when skip_store) on rows whose rowb >= 0; no bias.
// The training forward passes two more outputs, NULL otherwise: mode 0 keeps the two gate values in gate[m][0:2C], mode 1
// writes the updated residual rows to h_out (the next layer's own image) and leaves h as the backward pass needs it.
//
// Precision 0 is the exact-f32 MFMA (v_mfma_f32_32x32x2_f32), 1 split-bf16 x 3 and 2 plain bf16 on
// v_mfma_f32_32x32x16_bf16, with the operand splitting of gemm.hip's bf16 kernels.
#include "rowmma.h"

struct WgLayerParams {
    const float* X;
    long long ldx;
    const float* W;
    const float* bias;
    int M, N, K, Cin, taps, dil, mode;
    const float* cnd;
    long long ldcnd;
    float* acts;
    long long ldacts;
    float* h;
    long long ldh;
    int nres, skip_store;
    float* skip;
    long long ldskip;
    const int* rowb;
    float* gate;          // mode 0, optional: gate[m] = [tanh (C) | sigmoid (C)] kept for the backward pass
    long long ldgate;
    float* h_out;         // mode 1, optional: the updated residual rows go here instead of into h
    long long ldhout;
};

__device__ __forceinline__ float wg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Epilogue of one wave's 64 x 64 block: acc[tm][tn] is the 32 x 32 tile at rows wm*64 + tm*32, columns wn*64 + tn*32.
__device__ __forceinline__ void wg_layer_epilogue(const WgLayerParams& p, f32x16 (&acc)[2][2], int row0, int col0, int wm,
                                                  int wn, int lane) {
    const int l31 = lane & 31, lhi = lane >> 5;
    const int cbase = col0 + wn * 64;
    if (p.mode == 0) {
        if (cbase >= p.N) return;
        const int C = p.N >> 1;
        const int c = (cbase >> 1) + l31;
        const float bt = p.bias[cbase + l31], bs = p.bias[cbase + 32 + l31];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = row0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (gm < p.M) {
                    const float* cr = p.cnd + (long long)gm * p.ldcnd;
                    const float t = acc[tm][0][r] + bt + cr[c];
                    const float s = acc[tm][1][r] + bs + cr[C + c];
                    const float tt = tanhf(t), ss = wg_sigmoid(s);
                    p.acts[(long long)gm * p.ldacts + c] = tt * ss;
                    if (p.gate) {
                        p.gate[(long long)gm * p.ldgate + c] = tt;
                        p.gate[(long long)gm * p.ldgate + C + c] = ss;
                    }
                }
            }
        }
        return;
    }
    if (p.mode == 2) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int gn = cbase + tn * 32 + l31;
            if (gn >= p.N) continue;
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int gm = row0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    if (gm < p.M && p.rowb[gm] >= 0) {
                        float* hp = p.h + (long long)gm * p.ldh + gn;
                        *hp = p.skip_store ? acc[tm][tn][r] : *hp + acc[tm][tn][r];
                    }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int gn = cbase + tn * 32 + l31;
        if (gn >= p.N) continue;
        const float b = p.bias[gn];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = row0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (gm < p.M) {
                    const float v = acc[tm][tn][r] + b;
                    if (gn < p.nres) {
                        if (p.rowb[gm] >= 0) {
                            const float* hp = p.h + (long long)gm * p.ldh + gn;
                            float* ho = p.h_out ? p.h_out + (long long)gm * p.ldhout + gn : p.h + (long long)gm * p.ldh + gn;
                            *ho = *hp + v;
                        }
                    } else {
                        float* sp = p.skip + (long long)gm * p.ldskip + (gn - p.nres);
                        *sp = p.skip_store ? v : *sp + v;
                    }
                }
            }
        }
    }
}

// The rows of one 128 x 128 tile for csrc/rowmma.h: 32-bit row arithmetic, `gm < M` the only guard (the caller's halo covers
// every shifted row), the tap of a K-step taken once per step.
struct WgRows {
    const WgLayerParams& p;
    int row0, col0, half;
    __device__ __forceinline__ RmStep step(int k0) const {
        const int tap = k0 / p.Cin;
        return {(tap - half) * p.dil, k0 - tap * p.Cin};
    }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const int gm = row0 + r;
        return gm < p.M ? *reinterpret_cast<const float4*>(p.X + (long long)(gm + s.off) * p.ldx + s.col + kc)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[2][2], int wm, int wn, int lane) const {
        wg_layer_epilogue(p, acc, row0, col0, wm, wn, lane);
    }
};

// blockIdx.x = column tile, blockIdx.y = row tile: the column tiles of a row tile are neighbours in the launch order
__global__ __launch_bounds__(256) void wg_layer_f32_kernel(WgLayerParams p) {
    const WgRows rows{p, (int)blockIdx.y * 128, (int)blockIdx.x * 128, (p.taps - 1) / 2};
    rm_tile_f32<2, 2, 2, 2>(rows, p.W, p.N, p.K, rows.col0);
}

template <bool X3>
__global__ __launch_bounds__(256) void wg_layer_bf16_kernel(WgLayerParams p) {
    const WgRows rows{p, (int)blockIdx.y * 128, (int)blockIdx.x * 128, (p.taps - 1) / 2};
    rm_tile_bf16<X3, 2, 2, 2, 2>(rows, p.W, p.N, p.K, rows.col0);
}

extern "C" int t2amd_wg_layer_train_f32(const float* X, long long ldx, const float* W, const float* bias, int M, int N, int Cin,
                                        int taps, int dil, int mode, const float* cnd, long long ldcnd, float* acts,
                                        long long ldacts, float* h, long long ldh, int nres, float* skip, long long ldskip,
                                        int skip_store, const int* rowb, float* gate, long long ldgate, float* h_out,
                                        long long ldhout, int precision, void* stream) {
    T2_REQUIRE(X && W && (bias || mode == 2), "wg_layer: null operand");
    T2_REQUIRE(M > 0 && N > 0 && Cin > 0 && taps >= 1 && taps % 2 == 1 && dil >= 1, "wg_layer: bad dims");
    T2_REQUIRE(Cin % 32 == 0, "wg_layer: input channels must be a multiple of 32");
    T2_REQUIRE(ldx >= Cin && ldx % 4 == 0 && t2_aligned16(X) && t2_aligned16(W), "wg_layer: X / W must be 16-byte aligned rows");
    T2_REQUIRE(precision >= 0 && precision <= 2, "wg_layer: precision must be 0 (exact f32), 1 (split-bf16 x3) or 2 (bf16)");
    WgLayerParams p;
    p.X = X; p.ldx = ldx; p.W = W; p.bias = bias;
    p.M = M; p.N = N; p.K = taps * Cin; p.Cin = Cin; p.taps = taps; p.dil = dil; p.mode = mode;
    p.cnd = cnd; p.ldcnd = ldcnd; p.acts = acts; p.ldacts = ldacts;
    p.h = h; p.ldh = ldh; p.nres = nres; p.skip_store = skip_store; p.skip = skip; p.ldskip = ldskip; p.rowb = rowb;
    p.gate = gate; p.ldgate = ldgate; p.h_out = h_out; p.ldhout = ldhout;
    T2_REQUIRE(!gate || (mode == 0 && ldgate >= N), "wg_layer: gate values are kept by the gated product, 2C per row");
    T2_REQUIRE(!h_out || (mode == 1 && nres > 0 && ldhout >= nres), "wg_layer: h_out belongs to the residual columns");
    if (mode == 0) {
        T2_REQUIRE(cnd && acts, "wg_layer: gated product needs cnd and acts");
        T2_REQUIRE(N % 128 == 0, "wg_layer: gated product needs N = 2C with C a multiple of 64");
        T2_REQUIRE(ldcnd >= N && ldacts >= N / 2, "wg_layer: cnd / acts rows too short");
    } else if (mode == 1) {
        T2_REQUIRE(taps == 1, "wg_layer: residual / skip product is 1x1");
        T2_REQUIRE(skip && rowb, "wg_layer: residual / skip product needs skip and rowb");
        T2_REQUIRE(nres >= 0 && nres < N, "wg_layer: nres out of range");
        T2_REQUIRE(nres == 0 || (h && ldh >= nres), "wg_layer: residual columns need h");
        T2_REQUIRE(ldskip >= N - nres, "wg_layer: skip rows too short");
    } else if (mode == 2) {
        T2_REQUIRE(h && rowb && ldh >= N, "wg_layer: the data gradient needs h and rowb");
    } else {
        T2_FAIL("wg_layer: mode must be 0 (gated), 1 (residual / skip) or 2 (data gradient)");
    }
    dim3 grid(t2_cdiv(N, 128), t2_cdiv(M, 128));
    T2_REQUIRE(grid.y <= 65535, "wg_layer: too many rows");
    hipStream_t s = (hipStream_t)stream;
    rm_launch(precision, wg_layer_f32_kernel, wg_layer_bf16_kernel<true>, wg_layer_bf16_kernel<false>, grid, s, p);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_wg_layer_f32(const float* X, long long ldx, const float* W, const float* bias, int M, int N, int Cin,
                                  int taps, int dil, int mode, const float* cnd, long long ldcnd, float* acts,
                                  long long ldacts, float* h, long long ldh, int nres, float* skip, long long ldskip,
                                  int skip_store, const int* rowb, int precision, void* stream) {
    T2_REQUIRE(mode == 0 || mode == 1, "wg_layer: mode must be 0 (gated) or 1 (residual / skip)");
    return t2amd_wg_layer_train_f32(X, ldx, W, bias, M, N, Cin, taps, dil, mode, cnd, ldcnd, acts, ldacts, h, ldh, nres, skip,
                                    ldskip, skip_store, rowb, nullptr, 0, nullptr, 0, precision, stream);
}
