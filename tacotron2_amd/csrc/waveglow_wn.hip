// WaveGlow under weight norm (tacotron2_amd/waveglow.py: WaveGlow(weight_norm=True)): the fold w = g v / ||v|| of EVERY
// weight-normed tensor of the module in one launch, and its backward (dw -> dg, dv) in one launch, over a segment table.
// glow.py wraps start, in_layers, res_skip_layers and cond_layer in torch.nn.utils.weight_norm: 18 tensors per flow at
// 8 layers, 216 per module.  Plain C++ (sqrtf, __shfl_xor, no builtins, no atomics) so that the CPU test-suite can run
// these very kernels through tests/hip_emu; two runs give identical bits.
//
// The table, int64 [n_seg][WGN_COLS], one line per tensor (all offsets in floats from the base pointers):
//   [0] off    of the tensor in the v buffer, the w buffer and the dv buffer (the three share one layout)
//   [1] goff   of its first row in the g buffer, the norm buffer and the dg buffer
//   [2] dwoff  of its gradient in the dw buffer (WaveGlow._grad_layout: another layout)
//   [3] rows   output channels, [4] len  floats per row (C_in * kernel_size)
//   [5] first  work unit of the tensor: units are counted through the table in order
// A work unit is one wave: one row when len > WGN_SHORT, else 64 rows, one per lane (start's rows are 1 .. 4 floats).
// The sum order of a row depends on len alone: per lane the float4 (or float) elements lane, lane + 64, ... in order, then
// a xor butterfly over the wave (32, 16, .. 1), which leaves the same bits in every lane -- so a tensor's result does not
// depend on which other tensors share the table.  Rows of a multiple of 4 floats at offsets that are multiples of 4 move
// as 16-byte accesses and stay in registers between the reduction and the second pass (up to WGN_KEEP * 256 floats: 768
// covers in_layers; longer rows are read again).
#include "common.h"

#define WGN_COLS 6
#define WGN_WAVES 4          // waves (work units) per workgroup
#define WGN_SHORT 4          // rows of at most this many floats: one lane per row
#define WGN_KEEP 3           // float4 per lane kept in registers

// the table line that holds work unit u (first[s] <= u < first[s + 1]); n_seg >= 1 and u < n_units
__device__ __forceinline__ int wgn_find(const long long* __restrict__ table, int n_seg, long long u) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(long long)mid * WGN_COLS + 5] <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Every lane of every wave runs the butterflies (inactive ones with zeros): control flow around them is uniform.
__global__ void __launch_bounds__(64 * WGN_WAVES) wg_weight_norm_kernel(const long long* __restrict__ table, int n_seg,
                                                                        long long n_units, const float* __restrict__ v_base,
                                                                        const float* __restrict__ g_base,
                                                                        float* __restrict__ w_base, float* __restrict__ norm_base) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * WGN_WAVES + (threadIdx.x >> 6);
    const bool active = u < n_units;
    long long off = 0, goff = 0, rows = 0, len = 0, first = 0;
    if (active) {
        const long long* t = table + (long long)wgn_find(table, n_seg, u) * WGN_COLS;
        off = t[0], goff = t[1], rows = t[3], len = t[4], first = t[5];
    }
    const bool shortrow = len <= WGN_SHORT;
    const bool vec = active && !shortrow && (len & 3) == 0 && (off & 3) == 0;
    const long long r = shortrow ? (u - first) * 64 + lane : u - first;
    const float* v = v_base + off + r * len;
    float* w = w_base + off + r * len;
    const int nq = (int)(len >> 2);
    float4 keep[WGN_KEEP];
    float s = 0.0f;
    if (vec) {
        for (int t = 0; t < WGN_KEEP; ++t) {
            const int q = lane + 64 * t;
            if (q < nq) {
                keep[t] = *(const float4*)(v + 4 * q);
                s += keep[t].x * keep[t].x;
                s += keep[t].y * keep[t].y;
                s += keep[t].z * keep[t].z;
                s += keep[t].w * keep[t].w;
            }
        }
        for (int q = lane + 64 * WGN_KEEP; q < nq; q += 64) {
            const float4 x = *(const float4*)(v + 4 * q);
            s += x.x * x.x;
            s += x.y * x.y;
            s += x.z * x.z;
            s += x.w * x.w;
        }
    } else if (active && !shortrow) {
        for (long long j = lane; j < len; j += 64) s += v[j] * v[j];
    }
    s = t2_wave_sum(s);
    if (!active) return;
    if (shortrow) {
        if (r >= rows) return;
        float q = 0.0f;
        for (int j = 0; j < (int)len; ++j) q += v[j] * v[j];
        const float n = sqrtf(q);
        const float c = g_base[goff + r] / n;
        for (int j = 0; j < (int)len; ++j) w[j] = v[j] * c;
        norm_base[goff + r] = n;
        return;
    }
    const float n = sqrtf(s);
    const float c = g_base[goff + r] / n;
    if (vec) {
        for (int t = 0; t < WGN_KEEP; ++t) {
            const int q = lane + 64 * t;
            if (q < nq) *(float4*)(w + 4 * q) = make_float4(keep[t].x * c, keep[t].y * c, keep[t].z * c, keep[t].w * c);
        }
        for (int q = lane + 64 * WGN_KEEP; q < nq; q += 64) {
            const float4 x = *(const float4*)(v + 4 * q);
            *(float4*)(w + 4 * q) = make_float4(x.x * c, x.y * c, x.z * c, x.w * c);
        }
    } else {
        for (long long j = lane; j < len; j += 64) w[j] = v[j] * c;
    }
    if (lane == 0) norm_base[goff + r] = n;
}

// Per row, with n = norm[r] kept by the fold and d = sum_j dw[j] v[j] (the fold's reduction rule):
//   dg[r] = scale d / n,   dv[j] = scale (g[r] / n) (dw[j] - v[j] d / n^2)
__global__ void __launch_bounds__(64 * WGN_WAVES) wg_weight_norm_bwd_kernel(
    const long long* __restrict__ table, int n_seg, long long n_units, const float* __restrict__ dw_base,
    const float* __restrict__ v_base, const float* __restrict__ g_base, const float* __restrict__ norm_base,
    float* __restrict__ dg_base, float* __restrict__ dv_base, float scale) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * WGN_WAVES + (threadIdx.x >> 6);
    const bool active = u < n_units;
    long long off = 0, goff = 0, dwoff = 0, rows = 0, len = 0, first = 0;
    if (active) {
        const long long* t = table + (long long)wgn_find(table, n_seg, u) * WGN_COLS;
        off = t[0], goff = t[1], dwoff = t[2], rows = t[3], len = t[4], first = t[5];
    }
    const bool shortrow = len <= WGN_SHORT;
    const bool vec = active && !shortrow && (len & 3) == 0 && (off & 3) == 0 && (dwoff & 3) == 0;
    const long long r = shortrow ? (u - first) * 64 + lane : u - first;
    const float* v = v_base + off + r * len;
    const float* dw = dw_base + dwoff + r * len;
    float* dv = dv_base + off + r * len;
    const int nq = (int)(len >> 2);
    float4 kv[WGN_KEEP], kd[WGN_KEEP];
    float s = 0.0f;
    if (vec) {
        for (int t = 0; t < WGN_KEEP; ++t) {
            const int q = lane + 64 * t;
            if (q < nq) {
                kv[t] = *(const float4*)(v + 4 * q);
                kd[t] = *(const float4*)(dw + 4 * q);
                s += kd[t].x * kv[t].x;
                s += kd[t].y * kv[t].y;
                s += kd[t].z * kv[t].z;
                s += kd[t].w * kv[t].w;
            }
        }
        for (int q = lane + 64 * WGN_KEEP; q < nq; q += 64) {
            const float4 x = *(const float4*)(v + 4 * q);
            const float4 y = *(const float4*)(dw + 4 * q);
            s += y.x * x.x;
            s += y.y * x.y;
            s += y.z * x.z;
            s += y.w * x.w;
        }
    } else if (active && !shortrow) {
        for (long long j = lane; j < len; j += 64) s += dw[j] * v[j];
    }
    s = t2_wave_sum(s);
    if (!active) return;
    if (shortrow) {
        if (r >= rows) return;
        float d = 0.0f;
        for (int j = 0; j < (int)len; ++j) d += dw[j] * v[j];
        const float n = norm_base[goff + r];
        const float c = g_base[goff + r] / n * scale;
        const float e = d / (n * n);
        for (int j = 0; j < (int)len; ++j) dv[j] = c * (dw[j] - v[j] * e);
        dg_base[goff + r] = d / n * scale;
        return;
    }
    const float n = norm_base[goff + r];
    const float c = g_base[goff + r] / n * scale;
    const float e = s / (n * n);
    if (vec) {
        for (int t = 0; t < WGN_KEEP; ++t) {
            const int q = lane + 64 * t;
            if (q < nq)
                *(float4*)(dv + 4 * q) = make_float4(c * (kd[t].x - kv[t].x * e), c * (kd[t].y - kv[t].y * e),
                                                     c * (kd[t].z - kv[t].z * e), c * (kd[t].w - kv[t].w * e));
        }
        for (int q = lane + 64 * WGN_KEEP; q < nq; q += 64) {
            const float4 x = *(const float4*)(v + 4 * q);
            const float4 y = *(const float4*)(dw + 4 * q);
            *(float4*)(dv + 4 * q) = make_float4(c * (y.x - x.x * e), c * (y.y - x.y * e), c * (y.z - x.z * e), c * (y.w - x.w * e));
        }
    } else {
        for (long long j = lane; j < len; j += 64) dv[j] = c * (dw[j] - v[j] * e);
    }
    if (lane == 0) dg_base[goff + r] = s / n * scale;
}

extern "C" int t2amd_wg_weight_norm_short(void) { return WGN_SHORT; }

static int wgn_check(const long long* table, int n_seg, long long n_units, const void* const* ptrs, int nptr) {
    T2_REQUIRE(table, "wg_weight_norm: null table");
    T2_REQUIRE(n_seg > 0 && n_units > 0, "wg_weight_norm: empty table");
    T2_REQUIRE(((uintptr_t)table & 7) == 0, "wg_weight_norm: the table must be 8-byte aligned");
    for (int i = 0; i < nptr; ++i) {
        T2_REQUIRE(ptrs[i], "wg_weight_norm: null operand");
        T2_REQUIRE(((uintptr_t)ptrs[i] & 15) == 0, "wg_weight_norm: the buffers must be 16-byte aligned");
    }
    T2_REQUIRE((n_units + WGN_WAVES - 1) / WGN_WAVES <= 0x7fffffffLL, "wg_weight_norm: too many rows");
    return T2AMD_OK;
}

extern "C" int t2amd_wg_weight_norm_f32(const long long* table, int n_seg, long long n_units, const float* v_base,
                                        const float* g_base, float* w_base, float* norm_base, void* stream) {
    const void* ptrs[] = {v_base, g_base, w_base, norm_base};
    T2_PROPAGATE(wgn_check(table, n_seg, n_units, ptrs, 4));
    T2_LAUNCH(wg_weight_norm_kernel, dim3((unsigned)((n_units + WGN_WAVES - 1) / WGN_WAVES)), dim3(64 * WGN_WAVES), 0,
              (hipStream_t)stream, table, n_seg, n_units, v_base, g_base, w_base, norm_base);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_wg_weight_norm_bwd_f32(const long long* table, int n_seg, long long n_units, const float* dw_base,
                                            const float* v_base, const float* g_base, const float* norm_base, float* dg_base,
                                            float* dv_base, float scale, void* stream) {
    const void* ptrs[] = {dw_base, v_base, g_base, norm_base, dg_base, dv_base};
    T2_PROPAGATE(wgn_check(table, n_seg, n_units, ptrs, 6));
    T2_LAUNCH(wg_weight_norm_bwd_kernel, dim3((unsigned)((n_units + WGN_WAVES - 1) / WGN_WAVES)), dim3(64 * WGN_WAVES), 0,
              (hipStream_t)stream, table, n_seg, n_units, dw_base, v_base, g_base, norm_base, dg_base, dv_base, scale);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
