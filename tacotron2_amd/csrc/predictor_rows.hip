// The thin ends of a temporal predictor (tacotron2_amd/fastpitch.py): the projection of C channels onto
// 1 to 4 values per row and the embedding of 1 to 4 scalar tracks into C channels with k taps, with their gradients.  The
// ragged convolution of csrc/fft_block.hip takes only multiples of 32 channels on both sides, so these two are row kernels.
//   projection   one wave per row (b, t), float4 accesses; lane l takes the float4 chunks l, l + 64, .. ascending and chains
//                fmaf(w, h, .) from +0 over their components; the xor butterfly 32 .. 1 of t2_wave_sum; then bias + sum.
//   dh           dh(b, t, c) = the fmaf chain from +0 over p ascending of g(b, t, p) w(p, c).
//   embedding    per row and channel the fmaf chain from +0 over p ascending, then j ascending, of w(c, p, j) v(b, t + j - k/2, p),
//                over the frames inside [0, T_b) only (a tap outside is skipped); then bias + sum; then base + that.
//   dv           u(b, t', p, j) = sum_c w(c, p, j) g(b, t', c) in the projection's order (lane chains, butterfly);
//                dv(b, t, p) = the plain sum from +0 over j ascending of u(b, t - j + k/2, p, j) over rows inside the utterance.
//   sums         dw and db of both: P partial sums over the real rows p RP .. p RP + RP - 1 of the flattened (b, t) ascending
//                (FfbSumPlan; s = fmaf(g, h, s) for dw, s += g for db), then the partials added in ascending order from +0.
// Rows at and beyond an utterance's length are never read and every output row there is +0.  One writer per element, fixed
// orders, no atomics.  Plain C++, __shfl_xor only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "predictor.h"

#define PRED_ROWS 4                     /* waves (= rows) per workgroup */

__device__ __forceinline__ float pred_dot4(const float4 w, const float4 h, float a) {
    a = fmaf(w.x, h.x, a);
    a = fmaf(w.y, h.y, a);
    a = fmaf(w.z, h.z, a);
    return fmaf(w.w, h.w, a);
}

// grid (ceil(T / 4), B), 256 lanes: wave w takes row 4 blockIdx.x + w
__global__ void __launch_bounds__(64 * PRED_ROWS) pred_project_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                                      const float* __restrict__ bias, const int* __restrict__ len,
                                                                      int T_max, int C, int P, float* __restrict__ y) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * PRED_ROWS + wave;
    const bool inside = t < T_max, real = t < T;                            // uniform in the wave
    const long long r = (long long)b * T_max + (inside ? t : 0), row = r * C;
    const int nq = C >> 2;
    float acc[PRED_MAX_P] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (real)
        for (int q = lane; q < nq; q += 64) {
            const float4 hv = t2_ld4(h + row + 4 * q);
#pragma unroll
            for (int p = 0; p < PRED_MAX_P; ++p)
                if (p < P) acc[p] = pred_dot4(t2_ld4(w + (long long)p * C + 4 * q), hv, acc[p]);
        }
#pragma unroll
    for (int p = 0; p < PRED_MAX_P; ++p)
        if (p < P) acc[p] = t2_wave_sum(acc[p]);                            // every lane of the workgroup takes part
    if (!inside || lane >= P) return;
    const float s = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
    y[r * P + lane] = !real ? 0.0f : bias ? bias[lane] + s : s;
}

// grid (ceil(T / 4), B), 256 lanes
__global__ void __launch_bounds__(64 * PRED_ROWS) pred_project_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                                          const int* __restrict__ len, int T_max, int C, int P,
                                                                          float* __restrict__ dh) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * PRED_ROWS + wave;
    if (t >= T_max) return;
    const bool real = t < T;
    const long long r = (long long)b * T_max + t, row = r * C;
    const int nq = C >> 2;
    float gp[PRED_MAX_P] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int p = 0; p < PRED_MAX_P; ++p)
        if (real && p < P) gp[p] = g[r * P + p];
    for (int q = lane; q < nq; q += 64) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (real) {
#pragma unroll
            for (int p = 0; p < PRED_MAX_P; ++p)
                if (p < P) {
                    const float4 wv = t2_ld4(w + (long long)p * C + 4 * q);
                    o.x = fmaf(gp[p], wv.x, o.x);
                    o.y = fmaf(gp[p], wv.y, o.y);
                    o.z = fmaf(gp[p], wv.z, o.z);
                    o.w = fmaf(gp[p], wv.w, o.w);
                }
        }
        t2_st4(dh + row + 4 * q, o);
    }
}

// grid (ceil(C / 256), parts), 256 lanes: lane = column, blockIdx.y = partial sum over the rows n RP .. of the flattened (b, t);
// a part is [P][C] of dw then 4 floats of db
__global__ void __launch_bounds__(256) pred_project_sums_part_kernel(const float* __restrict__ g, const float* __restrict__ h,
                                                                     const int* __restrict__ len, int B, int T_max, int C, int P,
                                                                     long long RP, float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (c >= C) return;
    const long long rows = (long long)B * T_max, r0 = n * RP, r1 = r0 + RP < rows ? r0 + RP : rows;
    float s[PRED_MAX_P] = {0.0f, 0.0f, 0.0f, 0.0f}, s1[PRED_MAX_P] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (long long r = r0; r < r1; ++r) {
        const int b = (int)(r / T_max), t = (int)(r % T_max);
        const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
        if (t >= T) continue;
        const float hv = h[r * C + c];
#pragma unroll
        for (int p = 0; p < PRED_MAX_P; ++p)
            if (p < P) {
                const float gv = g[r * P + p];
                s[p] = fmaf(gv, hv, s[p]);
                s1[p] += gv;
            }
    }
    float* out = part + (long long)n * ((long long)P * C + 4);
#pragma unroll
    for (int p = 0; p < PRED_MAX_P; ++p) {
        if (p < P) out[(long long)p * C + c] = s[p];
        if (c == 0) out[(long long)P * C + p] = s1[p];
    }
}

// grid ceil((P C + P) / 256): the partial sums in ascending order, from +0
__global__ void __launch_bounds__(256) pred_project_sums_finish_kernel(const float* __restrict__ part, int parts, int C, int P,
                                                                       float* __restrict__ dw, float* __restrict__ db) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n_dw = (long long)P * C, stride = n_dw + 4;
    if (e >= n_dw + P) return;
    float s = 0.0f;
    for (int n = 0; n < parts; ++n) s += part[n * stride + e];
    if (e < n_dw) {
        if (dw) dw[e] = s;
    } else if (db) {
        db[e - n_dw] = s;
    }
}

// grid (ceil(T / 4), B), 256 lanes
__global__ void __launch_bounds__(64 * PRED_ROWS) pred_embed_kernel(const float* __restrict__ v, const float* __restrict__ image,
                                                                    const float* __restrict__ bias, const float* __restrict__ base,
                                                                    const int* __restrict__ len, int T_max, int C, int P, int k,
                                                                    float* __restrict__ y) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * PRED_ROWS + wave;
    if (t >= T_max) return;
    const bool real = t < T;
    const long long r0 = (long long)b * T_max, row = (r0 + t) * C;
    const int nq = C >> 2, half = k >> 1;
    for (int q = lane; q < nq; q += 64) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (real) {
            for (int p = 0; p < P; ++p)
                for (int j = 0; j < k; ++j) {
                    const int tt = t + j - half;
                    if (tt < 0 || tt >= T) continue;                        // the frame does not exist
                    const float vv = v[(r0 + tt) * P + p];
                    const float4 wv = t2_ld4(image + (long long)(p * k + j) * C + 4 * q);
                    o.x = fmaf(wv.x, vv, o.x);
                    o.y = fmaf(wv.y, vv, o.y);
                    o.z = fmaf(wv.z, vv, o.z);
                    o.w = fmaf(wv.w, vv, o.w);
                }
            if (bias) {
                const float4 c = t2_ld4(bias + 4 * q);
                o.x = c.x + o.x;
                o.y = c.y + o.y;
                o.z = c.z + o.z;
                o.w = c.w + o.w;
            }
            if (base) {
                const float4 a = t2_ld4(base + row + 4 * q);
                o.x = a.x + o.x;
                o.y = a.y + o.y;
                o.z = a.z + o.z;
                o.w = a.w + o.w;
            }
        }
        t2_st4(y + row + 4 * q, o);
    }
}

// grid (ceil(T / 4), B), 256 lanes: dbase = the gradient masked to the real rows; dv by P k wave sums per row
__global__ void __launch_bounds__(64 * PRED_ROWS) pred_embed_bwd_kernel(const float* __restrict__ g, const float* __restrict__ image,
                                                                        const int* __restrict__ len, int T_max, int C, int P, int k,
                                                                        float* __restrict__ dbase, float* __restrict__ dv) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * PRED_ROWS + wave;
    const bool inside = t < T_max, real = t < T;                            // uniform in the wave
    const long long r0 = (long long)b * T_max, r = r0 + (inside ? t : 0), row = r * C;
    const int nq = C >> 2, half = k >> 1;
    if (dbase && inside)
        for (int q = lane; q < nq; q += 64) t2_st4(dbase + row + 4 * q, real ? t2_ld4(g + row + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f));
    if (!dv) return;                                                        // uniform in the launch
    for (int p = 0; p < P; ++p) {
        float s = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int tt = t - j + half;
            const bool in = real && tt >= 0 && tt < T;
            float a = 0.0f;
            if (in) {
                const float* wrow = image + (long long)(p * k + j) * C;
                const float* grow = g + (r0 + tt) * C;
                for (int q = lane; q < nq; q += 64) a = pred_dot4(t2_ld4(wrow + 4 * q), t2_ld4(grow + 4 * q), a);
            }
            a = t2_wave_sum(a);                                             // every lane of the workgroup takes part
            if (in) s += a;
        }
        if (inside && lane == 0) dv[r * P + p] = s;                         // s stayed +0 on a row at or beyond T_b
    }
}

// grid (ceil(C / 256), parts, P k + 1), 256 lanes: lane = column, blockIdx.z = (p, j) of dw, or P k for the bias sum
__global__ void __launch_bounds__(256) pred_embed_sums_part_kernel(const float* __restrict__ g, const float* __restrict__ v,
                                                                   const int* __restrict__ len, int B, int T_max, int C, int P, int k,
                                                                   long long RP, float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, z = blockIdx.z;
    if (c >= C) return;
    const bool is_bias = z == P * k;
    const int p = is_bias ? 0 : z / k, off = is_bias ? 0 : z % k - (k >> 1);
    const long long rows = (long long)B * T_max, r0 = n * RP, r1 = r0 + RP < rows ? r0 + RP : rows;
    float s = 0.0f;
    for (long long r = r0; r < r1; ++r) {
        const int b = (int)(r / T_max), t = (int)(r % T_max);
        const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
        if (t >= T) continue;
        const float gv = g[r * C + c];
        if (is_bias) {
            s += gv;
            continue;
        }
        const int tt = t + off;
        if (tt < 0 || tt >= T) continue;
        s = fmaf(gv, v[((long long)b * T_max + tt) * P + p], s);
    }
    part[((long long)n * (P * k + 1) + z) * C + c] = s;
}

// grid ceil((P k + 1) C / 256): the partial sums in ascending order from +0, dw written as (C, P, k)
__global__ void __launch_bounds__(256) pred_embed_sums_finish_kernel(const float* __restrict__ part, int parts, int C, int P, int k,
                                                                     float* __restrict__ dw, float* __restrict__ db) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n_part = (long long)(P * k + 1) * C;
    if (e >= n_part) return;
    const int z = (int)(e / C), c = (int)(e % C);
    float s = 0.0f;
    for (int n = 0; n < parts; ++n) s += part[n * n_part + e];
    if (z < P * k) {
        if (dw) dw[(long long)c * P * k + z] = s;
    } else if (db) {
        db[c] = s;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
extern "C" int t2amd_predictor_limits(int* max_frames, int* max_channels, int* max_taps, int* max_tracks, int* max_batch) {
    T2_REQUIRE(max_frames && max_channels && max_taps && max_tracks && max_batch, "predictor: limits: null operand");
    *max_frames = PRED_MAX_T;
    *max_channels = PRED_MAX_C;
    *max_taps = PRED_MAX_TAPS;
    *max_tracks = PRED_MAX_P;
    *max_batch = PRED_MAX_B;
    return T2AMD_OK;
}

extern "C" int t2amd_predictor_workspace(int B, int T, int C, int P, int k, int which, long long* bytes) {
    T2_REQUIRE(bytes, "predictor: workspace: null operand");
    T2_REQUIRE(which >= 0 && which <= 2,
               "predictor: workspace: which must be 0 (forward and input gradients), 1 (projection sums) or 2 (embedding sums)");
    T2_PROPAGATE(pred_check("workspace", B, T, C, P, k));
    *bytes = which == 0 ? 0 : which == 1 ? pred_project_sum_bytes(B, T, C, P) : pred_embed_sum_bytes(B, T, C, P, k);
    return T2AMD_OK;
}

extern "C" int t2amd_pred_project_f32(const float* h, const float* w, const float* bias, const int* lengths, int B, int T, int C, int P,
                                      float* y, void* stream) {
    T2_PROPAGATE(pred_check("project", B, T, C, P, 1));
    T2_REQUIRE(h && w && y, "predictor: project: null operand");
    T2_REQUIRE(t2_aligned16(h) && t2_aligned16(w), "predictor: project: h and w must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C, ny = 4LL * B * T * P;
    T2_REQUIRE(!t2_overlap(y, ny, h, n) && !t2_overlap(y, ny, w, 4LL * P * C) && !(bias && t2_overlap(y, ny, bias, 4LL * P)),
               "predictor: project: the output must not overlap the inputs");
    T2_LAUNCH(pred_project_kernel, dim3((unsigned)t2_cdiv(T, PRED_ROWS), (unsigned)B), dim3(64 * PRED_ROWS), 0, (hipStream_t)stream, h, w,
              bias, lengths, T, C, P, y);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_pred_project_bwd_f32(const float* g, const float* w, const int* lengths, int B, int T, int C, int P, float* dh,
                                          void* stream) {
    T2_PROPAGATE(pred_check("project_bwd", B, T, C, P, 1));
    T2_REQUIRE(g && w && dh, "predictor: project_bwd: null operand");
    T2_REQUIRE(t2_aligned16(w) && t2_aligned16(dh), "predictor: project_bwd: w and dh must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C;
    T2_REQUIRE(!t2_overlap(dh, n, g, 4LL * B * T * P) && !t2_overlap(dh, n, w, 4LL * P * C),
               "predictor: project_bwd: the output must not overlap the inputs");
    T2_LAUNCH(pred_project_bwd_kernel, dim3((unsigned)t2_cdiv(T, PRED_ROWS), (unsigned)B), dim3(64 * PRED_ROWS), 0, (hipStream_t)stream, g,
              w, lengths, T, C, P, dh);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_pred_project_sums_f32(const float* g, const float* h, const int* lengths, int B, int T, int C, int P, float* dw,
                                           float* db, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(pred_check("project_sums", B, T, C, P, 1));
    T2_REQUIRE(g && h && ws && (dw || db), "predictor: project_sums: null operand");
    T2_REQUIRE(ws_bytes >= pred_project_sum_bytes(B, T, C, P),
               "predictor: project_sums: the workspace is smaller than t2amd_predictor_workspace asks for");
    T2_REQUIRE(t2_aligned16(ws), "predictor: project_sums: the workspace is not aligned to 16 bytes");
    const long long n = 4LL * B * T * C, ng = 4LL * B * T * P, nw = 4LL * P * C, nb = 4LL * P;
    T2_REQUIRE(!t2_overlap(ws, ws_bytes, g, ng) && !t2_overlap(ws, ws_bytes, h, n) && !(dw && t2_overlap(dw, nw, ws, ws_bytes)) &&
                   !(db && t2_overlap(db, nb, ws, ws_bytes)) && !(dw && db && t2_overlap(dw, nw, db, nb)) &&
                   !(dw && (t2_overlap(dw, nw, g, ng) || t2_overlap(dw, nw, h, n))) &&
                   !(db && (t2_overlap(db, nb, g, ng) || t2_overlap(db, nb, h, n))),
               "predictor: project_sums: outputs and workspace must not overlap the inputs or each other");
    const FfbSumPlan sp = ffb_sum_plan(B, T);
    float* part = reinterpret_cast<float*>(ws);
    T2_LAUNCH(pred_project_sums_part_kernel, dim3((unsigned)t2_cdiv(C, 256), (unsigned)sp.P), dim3(256), 0, (hipStream_t)stream, g, h,
              lengths, B, T, C, P, sp.RP, part);
    T2_LAUNCH(pred_project_sums_finish_kernel, dim3((unsigned)t2_cdiv((long long)P * C + P, 256)), dim3(256), 0, (hipStream_t)stream,
              (const float*)part, sp.P, C, P, dw, db);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_pred_embed_f32(const float* v, const float* image, const float* bias, const float* base, const int* lengths, int B,
                                    int T, int C, int P, int k, float* y, void* stream) {
    T2_PROPAGATE(pred_check("embed", B, T, C, P, k));
    T2_REQUIRE(v && image && y, "predictor: embed: null operand");
    T2_REQUIRE(t2_aligned16(image) && t2_aligned16(bias) && t2_aligned16(base) && t2_aligned16(y),
               "predictor: embed: the image, bias, base and y must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C;
    T2_REQUIRE(!t2_overlap(y, n, v, 4LL * B * T * P) && !t2_overlap(y, n, image, 4LL * P * k * C) && !(bias && t2_overlap(y, n, bias, 4LL * C)) &&
                   !(base && t2_overlap(y, n, base, n)),
               "predictor: embed: the output must not overlap the inputs");
    T2_LAUNCH(pred_embed_kernel, dim3((unsigned)t2_cdiv(T, PRED_ROWS), (unsigned)B), dim3(64 * PRED_ROWS), 0, (hipStream_t)stream, v, image,
              bias, base, lengths, T, C, P, k, y);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_pred_embed_bwd_f32(const float* g, const float* image, const int* lengths, int B, int T, int C, int P, int k,
                                        float* dbase, float* dv, void* stream) {
    T2_PROPAGATE(pred_check("embed_bwd", B, T, C, P, k));
    T2_REQUIRE(g && (dbase || dv) && (image || !dv), "predictor: embed_bwd: null operand");
    T2_REQUIRE(t2_aligned16(g) && t2_aligned16(image) && t2_aligned16(dbase),
               "predictor: embed_bwd: g, the image and dbase must be aligned to 16 bytes");
    const long long n = 4LL * B * T * C, nv = 4LL * B * T * P, ni = 4LL * P * k * C;
    T2_REQUIRE(!(dbase && (t2_overlap(dbase, n, g, n) || (image && t2_overlap(dbase, n, image, ni)))) &&
                   !(dv && (t2_overlap(dv, nv, g, n) || t2_overlap(dv, nv, image, ni))) && !(dbase && dv && t2_overlap(dbase, n, dv, nv)),
               "predictor: embed_bwd: the outputs must not overlap the inputs or each other");
    T2_LAUNCH(pred_embed_bwd_kernel, dim3((unsigned)t2_cdiv(T, PRED_ROWS), (unsigned)B), dim3(64 * PRED_ROWS), 0, (hipStream_t)stream, g,
              image, lengths, T, C, P, k, dbase, dv);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_pred_embed_sums_f32(const float* g, const float* v, const int* lengths, int B, int T, int C, int P, int k, float* dw,
                                         float* db, unsigned char* ws, long long ws_bytes, void* stream) {
    T2_PROPAGATE(pred_check("embed_sums", B, T, C, P, k));
    T2_REQUIRE(g && v && ws && (dw || db), "predictor: embed_sums: null operand");
    T2_REQUIRE(ws_bytes >= pred_embed_sum_bytes(B, T, C, P, k),
               "predictor: embed_sums: the workspace is smaller than t2amd_predictor_workspace asks for");
    T2_REQUIRE(t2_aligned16(ws), "predictor: embed_sums: the workspace is not aligned to 16 bytes");
    const long long n = 4LL * B * T * C, nv = 4LL * B * T * P, nw = 4LL * P * k * C, nb = 4LL * C;
    T2_REQUIRE(!t2_overlap(ws, ws_bytes, g, n) && !t2_overlap(ws, ws_bytes, v, nv) && !(dw && t2_overlap(dw, nw, ws, ws_bytes)) &&
                   !(db && t2_overlap(db, nb, ws, ws_bytes)) && !(dw && db && t2_overlap(dw, nw, db, nb)) &&
                   !(dw && (t2_overlap(dw, nw, g, n) || t2_overlap(dw, nw, v, nv))) &&
                   !(db && (t2_overlap(db, nb, g, n) || t2_overlap(db, nb, v, nv))),
               "predictor: embed_sums: outputs and workspace must not overlap the inputs or each other");
    const FfbSumPlan sp = ffb_sum_plan(B, T);
    float* part = reinterpret_cast<float*>(ws);
    T2_LAUNCH(pred_embed_sums_part_kernel, dim3((unsigned)t2_cdiv(C, 256), (unsigned)sp.P, (unsigned)(P * k + 1)), dim3(256), 0,
              (hipStream_t)stream, g, v, lengths, B, T, C, P, k, sp.RP, part);
    T2_LAUNCH(pred_embed_sums_finish_kernel, dim3((unsigned)t2_cdiv((long long)(P * k + 1) * C, 256)), dim3(256), 0, (hipStream_t)stream,
              (const float*)part, sp.P, C, P, k, dw, db);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
