// The feed-forward Transformer block, the MFMA-free half (tacotron2_amd/transformer.py): add + LayerNorm
// and its input gradient, the column sums (LayerNorm's dweight and dbias, a convolution's dbias), the ReLU mask of a gradient,
// the transposed gradient slab and the slice sum of the convolution's weight gradient, and the entries that launch nothing.
//   add + LN     one wave per row (b, t), float4 accesses; lane l takes the float4 chunks l, l + 64, .. ascending.  z = x + residual;
//                the lane sum adds (z0 + z1) + (z2 + z3) per chunk, the xor butterfly 32 .. 1 of t2_wave_sum, mean = sum / C; the
//                variance is the second pass' fmaf chain over d = z - mean, component by component, the butterfly, / C;
//                rstd = 1 / sqrtf(var + eps); y = fmaf(d rstd, weight, bias).  weight NULL: y = z, no statistics ("add and mask").
//   dz           per row: gw = g weight, xh = (z - mean) rstd, the lane chains s1 += gw and s2 = fmaf(gw, xh, s2), butterflies,
//                m1 = s1 / C, m2 = s2 / C, dz = fmaf(-xh, m2, gw - m1) rstd.
//   column sums  two passes: partial p sums the real rows p RP .. p RP + RP - 1 of the flattened (b, t) ascending (s1 += g,
//                s2 = fmaf(g, xh, s2)), then the partials are added in ascending order from +0.
// Rows at and beyond an utterance's length are never read and every output row there is +0.  One writer per element, fixed orders,
// no atomics.  Plain C++, __shfl_xor only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "fft_block.h"

#define FFB_LN_ROWS 4                   /* waves (= rows) per workgroup */

__device__ __forceinline__ float4 ffb_z(const float* x, const float* res, long long at) {
    float4 a = t2_ld4(x + at);
    if (res) {
        const float4 r = t2_ld4(res + at);
        a.x += r.x;
        a.y += r.y;
        a.z += r.z;
        a.w += r.w;
    }
    return a;
}

// grid (ceil(T / 4), B), 256 lanes: wave w takes row 4 blockIdx.x + w
__global__ void __launch_bounds__(64 * FFB_LN_ROWS) ffb_add_ln_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                                      const int* __restrict__ len, int T_max, int C, float eps,
                                                                      float* __restrict__ y, float* __restrict__ z,
                                                                      float* __restrict__ mean, float* __restrict__ rstd) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * FFB_LN_ROWS + wave;
    const bool inside = t < T_max, real = t < T;                            // uniform in the wave
    const long long row = ((long long)b * T_max + (inside ? t : 0)) * C;
    const int nq = C >> 2;
    float mu = 0.0f, rs = 0.0f;
    if (w) {
        float s = 0.0f;
        if (real)
            for (int q = lane; q < nq; q += 64) {
                const float4 a = ffb_z(x, res, row + 4 * q);
                s += (a.x + a.y) + (a.z + a.w);
            }
        mu = t2_wave_sum(s) / (float)C;                                     // every lane of the workgroup takes part
        float ss = 0.0f;
        if (real)
            for (int q = lane; q < nq; q += 64) {
                const float4 a = ffb_z(x, res, row + 4 * q);
                const float d0 = a.x - mu, d1 = a.y - mu, d2 = a.z - mu, d3 = a.w - mu;
                ss = fmaf(d0, d0, ss);
                ss = fmaf(d1, d1, ss);
                ss = fmaf(d2, d2, ss);
                ss = fmaf(d3, d3, ss);
            }
        rs = 1.0f / sqrtf(t2_wave_sum(ss) / (float)C + eps);
    }
    if (!inside) return;
    for (int q = lane; q < nq; q += 64) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), o = a;
        if (real) {
            a = ffb_z(x, res, row + 4 * q);
            o = a;
            if (w) {
                const float4 g = t2_ld4(w + 4 * q), c = t2_ld4(bias + 4 * q);
                o.x = fmaf((a.x - mu) * rs, g.x, c.x);
                o.y = fmaf((a.y - mu) * rs, g.y, c.y);
                o.z = fmaf((a.z - mu) * rs, g.z, c.z);
                o.w = fmaf((a.w - mu) * rs, g.w, c.w);
            }
        }
        t2_st4(y + row + 4 * q, o);
        if (z) t2_st4(z + row + 4 * q, a);
    }
    if (mean && lane == 0) {
        mean[(long long)b * T_max + t] = real ? mu : 0.0f;
        rstd[(long long)b * T_max + t] = real ? rs : 0.0f;
    }
}

// grid (ceil(T / 4), B), 256 lanes
__global__ void __launch_bounds__(64 * FFB_LN_ROWS) ffb_add_ln_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                          const float* __restrict__ w, const int* __restrict__ len,
                                                                          int T_max, int C, float* __restrict__ dz) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * FFB_LN_ROWS + wave;
    const bool inside = t < T_max, real = t < T;
    const long long r = (long long)b * T_max + (inside ? t : 0), row = r * C;
    const int nq = C >> 2;
    const float mu = real ? mean[r] : 0.0f, rs = real ? rstd[r] : 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
    if (real)
        for (int q = lane; q < nq; q += 64) {
            const float4 gv = t2_ld4(g + row + 4 * q), zv = t2_ld4(z + row + 4 * q), wv = t2_ld4(w + 4 * q);
            const float g0 = gv.x * wv.x, g1 = gv.y * wv.y, g2 = gv.z * wv.z, g3 = gv.w * wv.w;
            s1 += g0;
            s2 = fmaf(g0, (zv.x - mu) * rs, s2);
            s1 += g1;
            s2 = fmaf(g1, (zv.y - mu) * rs, s2);
            s1 += g2;
            s2 = fmaf(g2, (zv.z - mu) * rs, s2);
            s1 += g3;
            s2 = fmaf(g3, (zv.w - mu) * rs, s2);
        }
    const float m1 = t2_wave_sum(s1) / (float)C, m2 = t2_wave_sum(s2) / (float)C;
    if (!inside) return;
    for (int q = lane; q < nq; q += 64) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (real) {
            const float4 gv = t2_ld4(g + row + 4 * q), zv = t2_ld4(z + row + 4 * q), wv = t2_ld4(w + 4 * q);
            o.x = fmaf(-((zv.x - mu) * rs), m2, gv.x * wv.x - m1) * rs;
            o.y = fmaf(-((zv.y - mu) * rs), m2, gv.y * wv.y - m1) * rs;
            o.z = fmaf(-((zv.z - mu) * rs), m2, gv.z * wv.z - m1) * rs;
            o.w = fmaf(-((zv.w - mu) * rs), m2, gv.w * wv.w - m1) * rs;
        }
        t2_st4(dz + row + 4 * q, o);
    }
}

// grid (ceil(C / 256), P), 256 lanes: lane = column, blockIdx.y = partial sum over the rows p RP .. of the flattened (b, t)
__global__ void __launch_bounds__(256) ffb_colsum_part_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const int* __restrict__ len, int B, int T_max, int C, long long RP,
                                                              float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (c >= C) return;
    const long long rows = (long long)B * T_max, r0 = p * RP, r1 = r0 + RP < rows ? r0 + RP : rows;
    float s1 = 0.0f, s2 = 0.0f;
    for (long long r = r0; r < r1; ++r) {
        const int b = (int)(r / T_max), t = (int)(r % T_max);
        const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
        if (t >= T) continue;
        const float gv = g[r * C + c];
        s1 += gv;
        if (z) s2 = fmaf(gv, (z[r * C + c] - mean[r]) * rstd[r], s2);
    }
    part[((long long)p * 2 + 0) * C + c] = s1;
    part[((long long)p * 2 + 1) * C + c] = s2;
}

// grid ceil(C / 256): the partial sums in ascending order, from +0
__global__ void __launch_bounds__(256) ffb_colsum_finish_kernel(const float* __restrict__ part, int P, int C, float* __restrict__ dbias,
                                                                float* __restrict__ dweight) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s1 = 0.0f, s2 = 0.0f;
    for (int p = 0; p < P; ++p) {
        s1 += part[((long long)p * 2 + 0) * C + c];
        s2 += part[((long long)p * 2 + 1) * C + c];
    }
    if (dbias) dbias[c] = s1;
    if (dweight) dweight[c] = s2;
}

// grid (ceil(T C / 1024), B), 256 lanes, a float4 each: out = g where y > 0, +0 elsewhere and at and beyond the length
__global__ void __launch_bounds__(256) ffb_relu_mask_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                            const int* __restrict__ len, int T_max, int C, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;    // C is a multiple of 4: a float4 lies in one row
    if (e >= (long long)T_max * C) return;
    const long long at = (long long)b * T_max * C + e;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e / C < T) {
        const float4 gv = t2_ld4(g + at), yv = t2_ld4(y + at);
        o.x = yv.x > 0.0f ? gv.x : 0.0f;
        o.y = yv.y > 0.0f ? gv.y : 0.0f;
        o.z = yv.z > 0.0f ? gv.z : 0.0f;
        o.w = yv.w > 0.0f ? gv.w : 0.0f;
    }
    t2_st4(out + at, o);
}

// grid (ceil(L / 256), C, S): out[s][c][i] = g(b, t, c) of the reduction index q = s L + i = b Tp + t, zeros where no frame lies
__global__ void __launch_bounds__(256) ffb_transpose_kernel(const float* __restrict__ g, const int* __restrict__ len, int B, int T_max,
                                                            int C, int Tp, int L, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, s = blockIdx.z;
    if (i >= L) return;
    const long long q = (long long)s * L + i;
    const int b = (int)(q / Tp), t = (int)(q % Tp);
    float v = 0.0f;
    if (b < B) {
        const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
        if (t < T) v = g[((long long)b * T_max + t) * C + c];
    }
    out[((long long)s * C + c) * L + i] = v;
}

// grid ceil(k Cin Cout / 256): dw(o, i, j) = the slices' partials [s][j Cin + i][o] added in ascending order
__global__ void __launch_bounds__(256) ffb_dw_finish_kernel(const float* __restrict__ part, int S, int Cin, int Cout, int k,
                                                            float* __restrict__ dw) {
    const long long n = (long long)k * Cin * Cout, e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int row = (int)(e / Cout), o = (int)(e % Cout);
    float a = part[e];
    for (int s = 1; s < S; ++s) a += part[s * n + e];
    dw[((long long)o * Cin + row % Cin) * k + row / Cin] = a;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
extern "C" int t2amd_fft_block_limits(int* max_frames, int* max_channels, int* max_taps, int* min_norm_channels, int* max_batch) {
    T2_REQUIRE(max_frames && max_channels && max_taps && min_norm_channels && max_batch, "fft_block: limits: null operand");
    *max_frames = FFB_MAX_T;
    *max_channels = FFB_MAX_C;
    *max_taps = FFB_MAX_TAPS;
    *min_norm_channels = FFB_MIN_LN;
    *max_batch = FFB_MAX_B;
    return T2AMD_OK;
}

extern "C" int t2amd_fft_block_workspace(int B, int T, int Cin, int Cout, int k, int which, long long* bytes) {
    T2_REQUIRE(bytes, "fft_block: workspace: null operand");
    T2_REQUIRE(which >= 0 && which <= 2, "fft_block: workspace: which must be 0 (convolution), 1 (weight gradient) or 2 (column sums)");
    if (which == 2) {
        T2_PROPAGATE(ffb_check_rows("workspace", B, T, Cout, 4));
        *bytes = ffb_sum_bytes(B, T, Cout);
        return T2AMD_OK;
    }
    T2_PROPAGATE(ffb_check_conv("workspace", B, T, Cin, Cout, k));
    *bytes = which == 0 ? 0 : ffb_dw_ws(B, T, Cin, Cout, k).bytes;
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_add_ln_f32(const float* x, const float* residual, const float* weight, const float* bias, const int* lengths,
                                    int B, int T, int C, float eps, float* y, float* z, float* mean, float* rstd, void* stream) {
    T2_PROPAGATE(ffb_check_rows("add_ln", B, T, C, FFB_MIN_LN));
    T2_REQUIRE(x && y && (!weight == !bias) && (!mean == !rstd) && (weight || !mean), "fft_block: add_ln: null operand");
    T2_REQUIRE(eps > 0.0f && eps <= 3.0e38f, "fft_block: add_ln: eps must be positive and finite");
    T2_REQUIRE(t2_aligned16(x) && t2_aligned16(y) && t2_aligned16(residual) && t2_aligned16(weight) && t2_aligned16(bias) && t2_aligned16(z),
               "fft_block: add_ln: operands must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C, nr = 4LL * B * T;
    T2_REQUIRE(!t2_overlap(y, n, x, n) && !(residual && t2_overlap(y, n, residual, n)) && !(weight && t2_overlap(y, n, weight, 4LL * C)) &&
                   !(bias && t2_overlap(y, n, bias, 4LL * C)) &&
                   !(z && (t2_overlap(z, n, x, n) || t2_overlap(z, n, y, n) || (residual && t2_overlap(z, n, residual, n)))) &&
                   !(mean && (t2_overlap(mean, nr, rstd, nr) || t2_overlap(mean, nr, x, n) || t2_overlap(rstd, nr, x, n) ||
                              t2_overlap(mean, nr, y, n) || t2_overlap(rstd, nr, y, n))),
               "fft_block: add_ln: the outputs must not overlap the inputs or each other");
    T2_LAUNCH(ffb_add_ln_kernel, dim3((unsigned)t2_cdiv(T, FFB_LN_ROWS), (unsigned)B), dim3(64 * FFB_LN_ROWS), 0, (hipStream_t)stream, x,
              residual, weight, bias, lengths, T, C, eps, y, z, mean, rstd);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_add_ln_bwd_f32(const float* g, const float* z, const float* mean, const float* rstd, const float* weight,
                                        const int* lengths, int B, int T, int C, float* dz, void* stream) {
    T2_PROPAGATE(ffb_check_rows("add_ln_bwd", B, T, C, FFB_MIN_LN));
    T2_REQUIRE(g && z && mean && rstd && weight && dz, "fft_block: add_ln_bwd: null operand");
    T2_REQUIRE(t2_aligned16(g) && t2_aligned16(z) && t2_aligned16(weight) && t2_aligned16(dz),
               "fft_block: add_ln_bwd: operands must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C, nr = 4LL * B * T;
    T2_REQUIRE(!t2_overlap(dz, n, g, n) && !t2_overlap(dz, n, z, n) && !t2_overlap(dz, n, mean, nr) && !t2_overlap(dz, n, rstd, nr) &&
                   !t2_overlap(dz, n, weight, 4LL * C),
               "fft_block: add_ln_bwd: the output must not overlap the inputs");
    T2_LAUNCH(ffb_add_ln_bwd_kernel, dim3((unsigned)t2_cdiv(T, FFB_LN_ROWS), (unsigned)B), dim3(64 * FFB_LN_ROWS), 0, (hipStream_t)stream,
              g, z, mean, rstd, weight, lengths, T, C, dz);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_colsum_f32(const float* g, const float* z, const float* mean, const float* rstd, const int* lengths, int B,
                                    int T, int C, float* dbias, float* dweight, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(ffb_check_rows("colsum", B, T, C, 4));
    T2_REQUIRE(g && ws && (dbias || dweight) && (z ? (mean && rstd) : !dweight), "fft_block: colsum: null operand");
    T2_REQUIRE(ws_bytes >= ffb_sum_bytes(B, T, C), "fft_block: colsum: the workspace is smaller than t2amd_fft_block_workspace asks for");
    T2_REQUIRE(t2_aligned16(ws), "fft_block: colsum: the workspace is not aligned to 16 bytes");
    const long long n = 4LL * B * T * C;
    T2_REQUIRE(!t2_overlap(ws, ws_bytes, g, n) && !(z && t2_overlap(ws, ws_bytes, z, n)) && !(dbias && t2_overlap(dbias, 4LL * C, ws, ws_bytes)) &&
                   !(dweight && t2_overlap(dweight, 4LL * C, ws, ws_bytes)) && !(dbias && dweight && t2_overlap(dbias, 4LL * C, dweight, 4LL * C)) &&
                   !(dbias && t2_overlap(dbias, 4LL * C, g, n)) && !(dweight && t2_overlap(dweight, 4LL * C, g, n)),
               "fft_block: colsum: outputs and workspace must not overlap the inputs or each other");
    const FfbSumPlan sp = ffb_sum_plan(B, T);
    float* part = reinterpret_cast<float*>(ws);
    T2_LAUNCH(ffb_colsum_part_kernel, dim3((unsigned)t2_cdiv(C, 256), (unsigned)sp.P), dim3(256), 0, (hipStream_t)stream, g, z, mean, rstd,
              lengths, B, T, C, sp.RP, part);
    T2_LAUNCH(ffb_colsum_finish_kernel, dim3((unsigned)t2_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)part, sp.P, C, dbias,
              dweight);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_relu_mask_f32(const float* g, const float* y, const int* lengths, int B, int T, int C, float* out, void* stream) {
    T2_PROPAGATE(ffb_check_rows("relu_mask", B, T, C, 4));
    T2_REQUIRE(g && y && out, "fft_block: relu_mask: null operand");
    T2_REQUIRE(t2_aligned16(g) && t2_aligned16(y) && t2_aligned16(out), "fft_block: relu_mask: operands must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C;
    T2_REQUIRE(!t2_overlap(out, n, g, n) && !t2_overlap(out, n, y, n), "fft_block: relu_mask: the output must not overlap the inputs");
    T2_LAUNCH(ffb_relu_mask_kernel, dim3((unsigned)t2_cdiv((long long)T * C, 1024), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, y,
              lengths, T, C, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_transpose_f32(const float* g, const int* lengths, int B, int T, int C, float* out, long long out_bytes, void* stream) {
    T2_PROPAGATE(ffb_check_rows("transpose", B, T, C, 4));
    T2_REQUIRE(g && out, "fft_block: transpose: null operand");
    const FfbDwPlan d = ffb_dw_plan(B, T);
    T2_REQUIRE(out_bytes >= 4LL * d.S * C * d.L, "fft_block: transpose: the slab is smaller than its slices");
    T2_REQUIRE(t2_aligned16(out), "fft_block: transpose: the slab is not aligned to 16 bytes");
    T2_REQUIRE(!t2_overlap(out, out_bytes, g, 4LL * B * T * C), "fft_block: transpose: the slab must not overlap the input");
    T2_LAUNCH(ffb_transpose_kernel, dim3((unsigned)t2_cdiv(d.L, 256), (unsigned)C, (unsigned)d.S), dim3(256), 0, (hipStream_t)stream, g, lengths,
              B, T, C, d.Tp, d.L, out);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_ffb_dw_finish_f32(const float* part, int slices, int Cin, int Cout, int k, float* dw, void* stream) {
    T2_PROPAGATE(ffb_check_conv("dw_finish", 1, 1, Cin, Cout, k));
    T2_REQUIRE(part && dw, "fft_block: dw_finish: null operand");
    T2_REQUIRE(slices >= 1 && slices <= FFB_DW_MAX_SLICES, "fft_block: dw_finish: 1 to 8 slices");
    const long long n = 4LL * k * Cin * Cout;
    T2_REQUIRE(!t2_overlap(dw, n, part, n * slices), "fft_block: dw_finish: the output must not overlap the partials");
    T2_LAUNCH(ffb_dw_finish_kernel, dim3((unsigned)t2_cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, part, slices, Cin, Cout, k, dw);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
