// The feed-forward Transformer block's ragged convolution, the two dense products (tacotron2_amd/transformer.py, DESIGN.md
// section 23), on the MFMA tile loop of csrc/rowmma.h: rm_tile_f32 clients (v_mfma_f32_32x32x2_f32, exact f32, every sum over the
// reduction index ascending) with their own Rows policies, 128 x BN tiles with BN = the widest of 128, 64, 32 that divides the
// column count, blockIdx.z = utterance (convolution) or reduction slice (weight gradient).
//   1. y[t][o]  = act(bias[o] + sum_{j, i} image[o][j Cin + i] x[t + j - k/2][i])    A = the utterance's own rows, shifted by the
//                 step's tap, zero where t + j - k/2 lies outside [0, T_b); reduction over K = k Cin, tap-major.  The epilogue
//                 adds the bias, applies ReLU, keeps the value only where a second tensor is positive (the ReLU of the layer
//                 below, for dx), and stores +0 on the rows at and beyond T_b.  dx is the same kernel on the image of the
//                 flipped, transposed weights.
//   2. part[s][j Cin + i][o] = sum over the slice's q = b Tp + t of x[b][t + j - k/2][i] g[b][t][o]    A = x read down its
//                 columns, tap-shifted (a strided policy, zero outside the utterance), B = the slice's slab gT [Cout][L] of
//                 csrc/fft_block_rows.hip; the slices are added in ascending order by ffb_dw_finish_kernel.
// What lies beyond an utterance's count is zero in an operand, and adding +0 to a sum that started at +0 changes no bit, so an
// utterance in a ragged batch gives the bits it gives alone.  One writer per element, no atomics.
#include "fft_block.h"
#include "rowmma.h"

struct FfbConv {
    const float* x;                     // (B, T_max, Cin) at strides xb, xt
    long long xb, xt;
    const float* W;                     // 1: the weight image [Cout][k Cin]; 2: the slabs gT, S of [Cout][L]
    const float* bias;                  // 1: [Cout] or null
    const float* mask;                  // 1: (B, T_max, Cout) or null: keep y only where it is positive
    float* out;                         // 1: y (B, T_max, Cout); 2: the partials, S of [k Cin][Cout]
    const int* len;
    int B, T_max, Cin, Cout, k, relu, Tp, L;
};

#define FFB_FOR_TILE(TM, TN, body)                                                                                         \
    _Pragma("unroll") for (int tn = 0; tn < TN; ++tn) {                                                                    \
        const int gn = col0 + (wn * TN + tn) * 32 + (lane & 31);                                                           \
        _Pragma("unroll") for (int tm = 0; tm < TM; ++tm) _Pragma("unroll") for (int r = 0; r < 16; ++r) {                 \
            const int gm = row0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);                          \
            const float v = acc[tm][tn][r];                                                                                \
            body                                                                                                           \
        }                                                                                                                  \
    }

struct FfbConvRows {
    const float* x;                     // the utterance's rows
    long long xt;
    int Cin, half, T, T_max, Cout, row0, col0, relu;
    float* y;                           // the utterance's [T_max][Cout]
    const float* bias;
    const float* mask;
    __device__ __forceinline__ RmStep step(int k0) const {
        const int j = k0 / Cin;
        return {j - half, k0 - j * Cin};
    }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const int t = row0 + r + s.off;
        return (t >= 0 && t < T) ? t2_ld4(x + t * xt + s.col + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        FFB_FOR_TILE(TM, TN, if (gm < T_max && gn < Cout) {
            float o = 0.0f;
            if (gm < T) {
                o = bias ? v + bias[gn] : v;
                if (relu) o = o > 0.0f ? o : 0.0f;
                if (mask) o = mask[(long long)gm * Cout + gn] > 0.0f ? o : 0.0f;
            }
            y[(long long)gm * Cout + gn] = o;
        })
    }
};

struct FfbDwRows {
    const float* x;
    long long xb, xt;
    const int* len;
    int B, T_max, Cin, R, half, Tp, q0, Cout, row0, col0;
    float* part;                        // the slice's [R][Cout]
    __device__ __forceinline__ RmStep step(int k0) const { return {0, k0}; }
    __device__ __forceinline__ float4 a(const RmStep& s, int r, int kc) const {
        const int row = row0 + r, q = q0 + s.col + kc;                      // q is a multiple of 4 and Tp of 32: one utterance
        const int b = q / Tp, t = q - b * Tp;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row >= R || b >= B) return o;
        const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
        const int j = row / Cin, i = row - j * Cin;
        const float* p = x + b * xb + i;
        const int u = t + j - half;                                         // the frame of x under frame t of g
        if (t + 0 < T && u + 0 >= 0 && u + 0 < T) o.x = p[(u + 0) * xt];
        if (t + 1 < T && u + 1 >= 0 && u + 1 < T) o.y = p[(u + 1) * xt];
        if (t + 2 < T && u + 2 >= 0 && u + 2 < T) o.z = p[(u + 2) * xt];
        if (t + 3 < T && u + 3 >= 0 && u + 3 < T) o.w = p[(u + 3) * xt];
        return o;
    }
    template <int TM, int TN>
    __device__ __forceinline__ void epilogue(f32x16 (&acc)[TM][TN], int wm, int wn, int lane) const {
        FFB_FOR_TILE(TM, TN, if (gm < R && gn < Cout) part[(long long)gm * Cout + gn] = v;)
    }
};

// blockIdx.x = row tile of 128 frames, blockIdx.y = column tile, blockIdx.z = utterance
template <int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void ffb_conv_kernel(FfbConv p) {
    constexpr int BN = WNW * TN * 32;
    const int b = blockIdx.z, row0 = blockIdx.x * 128, col0 = blockIdx.y * BN;
    const int T = p.len ? t2_clamp_count(p.len[b], p.T_max) : p.T_max;
    float* y = p.out + (long long)b * p.T_max * p.Cout;
    if (row0 >= T) {                                                        // uniform: a tile wholly beyond the utterance
        for (int i = threadIdx.x; i < 128 * BN; i += 256) {
            const int gm = row0 + i / BN, gn = col0 + i % BN;
            if (gm < p.T_max && gn < p.Cout) y[(long long)gm * p.Cout + gn] = 0.0f;
        }
        return;
    }
    const FfbConvRows rows{p.x + b * p.xb, p.xt, p.Cin, p.k / 2, T, p.T_max, p.Cout, row0, col0, p.relu, y, p.bias,
                           p.mask ? p.mask + (long long)b * p.T_max * p.Cout : nullptr};
    rm_tile_f32<WMW, WNW, TM, TN>(rows, p.W, p.Cout, p.k * p.Cin, col0);
}

// blockIdx.x = row tile of 128 (tap, input channel) rows, blockIdx.y = column tile of output channels, blockIdx.z = slice
template <int WMW, int WNW, int TM, int TN>
__global__ __launch_bounds__(256) void ffb_conv_dw_kernel(FfbConv p) {
    constexpr int BN = WNW * TN * 32;
    const int s = blockIdx.z, row0 = blockIdx.x * 128, col0 = blockIdx.y * BN, R = p.k * p.Cin;
    const FfbDwRows rows{p.x, p.xb, p.xt, p.len, p.B, p.T_max, p.Cin, R, p.k / 2, p.Tp, s * p.L, p.Cout, row0, col0,
                         p.out + (long long)s * R * p.Cout};
    rm_tile_f32<WMW, WNW, TM, TN>(rows, p.W + (long long)s * p.Cout * p.L, p.Cout, p.L, col0);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static void ffb_launch(void (*kern)(FfbConv), dim3 grid, hipStream_t s, const FfbConv& p) { T2_LAUNCH(kern, grid, dim3(256), 0, s, p); }

// the three tile shapes of RM_LAUNCH_COLS, for a family of one precision
#define FFB_LAUNCH_COLS(KERN, BN, grid, s, p)                                                                              \
    do {                                                                                                                   \
        if ((BN) == 128)                                                                                                   \
            ffb_launch(KERN<2, 2, 2, 2>, grid, s, p);                                                                      \
        else if ((BN) == 64)                                                                                               \
            ffb_launch(KERN<2, 2, 2, 1>, grid, s, p);                                                                      \
        else                                                                                                               \
            ffb_launch(KERN<4, 1, 1, 1>, grid, s, p);                                                                      \
    } while (0)

extern "C" int t2amd_ffb_conv_f32(const float* x, long long xb, long long xt, const float* image, const float* bias, const float* mask,
                                  const int* lengths, int B, int T, int Cin, int Cout, int k, int relu, float* y, void* stream) {
    T2_PROPAGATE(ffb_check_conv("conv", B, T, Cin, Cout, k));
    T2_PROPAGATE(ffb_check_x("conv", x, xb, xt, B, T, Cin));
    T2_REQUIRE(image && y, "fft_block: conv: null operand");
    T2_REQUIRE(t2_aligned16(image) && t2_aligned16(y), "fft_block: conv: the weight image and y must be aligned to 16 bytes");
    const long long ybytes = 4LL * B * T * Cout;
    T2_REQUIRE(!t2_overlap(y, ybytes, x, t2_span_bytes(xb, xt, B, T, Cin)) && !t2_overlap(y, ybytes, image, 4LL * Cout * k * Cin) &&
                   !(bias && t2_overlap(y, ybytes, bias, 4LL * Cout)) && !(mask && t2_overlap(y, ybytes, mask, ybytes)),
               "fft_block: conv: y must not overlap the inputs");
    FfbConv p = {};
    p.x = x; p.xb = xb; p.xt = xt; p.W = image; p.bias = bias; p.mask = mask; p.out = y; p.len = lengths;
    p.B = B; p.T_max = T; p.Cin = Cin; p.Cout = Cout; p.k = k; p.relu = relu != 0;
    const int BN = rm_tile_cols(Cout);
    const dim3 grid((unsigned)t2_cdiv(T, 128), (unsigned)(Cout / BN), (unsigned)B);
    FFB_LAUNCH_COLS(ffb_conv_kernel, BN, grid, (hipStream_t)stream, p);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_conv_dw_f32(const float* g, const float* x, long long xb, long long xt, const int* lengths, int B, int T, int Cin,
                                     int Cout, int k, float* dw, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(ffb_check_conv("conv_dw", B, T, Cin, Cout, k));
    T2_PROPAGATE(ffb_check_x("conv_dw", x, xb, xt, B, T, Cin));
    T2_REQUIRE(g && dw && ws, "fft_block: conv_dw: null operand");
    const FfbDwWs w = ffb_dw_ws(B, T, Cin, Cout, k);
    T2_REQUIRE(ws_bytes >= w.bytes, "fft_block: conv_dw: the workspace is smaller than t2amd_fft_block_workspace asks for");
    T2_REQUIRE(t2_aligned16(ws) && t2_aligned16(g), "fft_block: conv_dw: the workspace and g must be aligned to 16 bytes");
    const long long gbytes = 4LL * B * T * Cout, wbytes = 4LL * Cout * Cin * k, xbytes = t2_span_bytes(xb, xt, B, T, Cin);
    T2_REQUIRE(!t2_overlap(ws, ws_bytes, g, gbytes) && !t2_overlap(ws, ws_bytes, x, xbytes) && !t2_overlap(dw, wbytes, ws, ws_bytes) &&
                   !t2_overlap(dw, wbytes, g, gbytes) && !t2_overlap(dw, wbytes, x, xbytes),
               "fft_block: conv_dw: dw and the workspace must not overlap the inputs or each other");
    const FfbDwPlan d = ffb_dw_plan(B, T);
    float* gT = reinterpret_cast<float*>(ws + w.gt);
    float* part = reinterpret_cast<float*>(ws + w.part);
    T2_PROPAGATE(t2amd_ffb_transpose_f32(g, lengths, B, T, Cout, gT, w.part, stream));
    FfbConv p = {};
    p.x = x; p.xb = xb; p.xt = xt; p.W = gT; p.out = part; p.len = lengths;
    p.B = B; p.T_max = T; p.Cin = Cin; p.Cout = Cout; p.k = k; p.Tp = d.Tp; p.L = d.L;
    const int BN = rm_tile_cols(Cout);
    const dim3 grid((unsigned)t2_cdiv((long long)k * Cin, 128), (unsigned)(Cout / BN), (unsigned)d.S);
    FFB_LAUNCH_COLS(ffb_conv_dw_kernel, BN, grid, (hipStream_t)stream, p);
    T2_LAUNCH_CHECK();
    return t2amd_ffb_dw_finish_f32(part, d.S, Cin, Cout, k, dw, stream);
}
