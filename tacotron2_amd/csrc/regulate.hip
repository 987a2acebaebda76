// The length regulator (tacotron2_amd/alignment.py; FastSpeech, FastPitch): durations -> the token of every
// frame, the expansion of token vectors to frame rate with its gradient (a segment sum), and the pooling of a frame-rate
// quantity over each token's frames with its gradient (a segment broadcast).
//   ends      e(n) = d(0) + .. + d(n) in 64 bits (a term saturates at 2^31 - 1), clamped to T; S = e(N_b - 1), T_b = min(S, T).
//   path      path(t) = the smallest n < N_b with e(n) > t for t < T_b, -1 for T_b <= t < T: a token with d = 0 owns no frame.
//   expand    y(t, :) = x(path(t), :) for t < T_b, +0 beyond: a copy, every bit comes through.
//   segsum    dx(n, :) = dy(e(n-1), :) + dy(e(n-1) + 1, :) + .., plain adds from the first term, t ascending; +0 without a frame.
//   pool      num(n) = fmaf(w(t), v(t), num) from +0, den(n) = den + w(t) from +0, t ascending over the token's frames below T;
//             m(n) = num / den where den > 0, +0 elsewhere.  Without weights w = 1.
//   pool bwd  dv(t) = w(t) * (g(path(t)) / den(path(t))): one division, one product; +0 where den = 0 and at and beyond T_b.
// An utterance with a negative duration below its N_b is marked: t_lengths = -1, every end 0, every path entry -1, so that
// whatever reads them writes zeros.  Durations at and beyond N_b are never read.
// Layout: the path kernel is one workgroup per utterance (a scan of 256 four-token sums in LDS, then a binary search per frame
// over the ends in LDS).  The per-frame kernels (expand, pool bwd) give a workgroup a run of frames and their lanes run along
// C; the per-token kernels (segsum, pool) give `width` lanes (a power of two, C rounded up, at most 64) to a token, the lanes
// run along C and walk the token's own frames in ascending order.  One writer per element, a fixed order, no atomics, no
// cross-lane sums: two calls give the same bits and an utterance in a ragged batch gives the bits it gives alone.  Plain C++
// and __syncthreads only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define RG_W 256                        /* lanes of a workgroup */
#define RG_MAX_N 1024                   /* tokens at most: RG_W lanes, four tokens each */
#define RG_MAX_T 65536                  /* frames at most */
#define RG_MAX_C 512                    /* channels at most */
#define RG_MAX_B 65535                  /* utterances: grid.y */
#define RG_ITEMS 2048                   /* elements (or groups of four) of a workgroup of the per-frame kernels */
#define RG_SAT 2147483647LL             /* a duration counts as at most this */

template <class D>
__global__ void __launch_bounds__(RG_W) regulate_path_kernel(const D* __restrict__ durations, long long db,
                                                             const int* __restrict__ n_len, int N_max, int T,
                                                             int* __restrict__ path, int* __restrict__ t_lengths,
                                                             int* __restrict__ ends_out, long long* __restrict__ totals) {
    __shared__ long long part[2][RG_W];
    __shared__ int ends[RG_MAX_N];
    __shared__ int bad;
    const int b = blockIdx.x, l = threadIdx.x;
    const int N = n_len ? t2_clamp_count(n_len[b], N_max) : N_max;
    const D* d = durations + b * db;
    long long own[4], sum = 0;
    bool neg = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = 4 * l + k;
        long long v = n < N ? (long long)d[n] : 0;
        neg = neg || v < 0;
        v = v < 0 ? 0 : v > RG_SAT ? RG_SAT : v;
        sum += v;
        own[k] = sum;
    }
    if (l == 0) bad = 0;
    part[0][l] = sum;
    __syncthreads();
    if (neg) bad = 1;                                                       // every writer writes the same value
    int cur = 0;
    for (int step = 1; step < RG_W; step <<= 1) {                           // an inclusive scan of the 256 sums
        const long long v = part[cur][l] + (l >= step ? part[cur][l - step] : 0);
        part[cur ^ 1][l] = v;
        cur ^= 1;
        __syncthreads();
    }
    const bool marked = bad != 0;                                           // uniform
    const long long before = l > 0 ? part[cur][l - 1] : 0;
    const long long S = marked ? 0 : part[cur][RG_W - 1];
    const int Tb = S < (long long)T ? (int)S : T;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = 4 * l + k;
        const long long e = before + own[k];
        if (n < RG_MAX_N) ends[n] = marked ? 0 : e < (long long)T ? (int)e : T;
    }
    __syncthreads();
    if (l == 0) {
        t_lengths[b] = marked ? -1 : Tb;
        if (totals) totals[b] = marked ? -1 : part[cur][RG_W - 1];
    }
    if (ends_out)
        for (int n = l; n < N_max; n += RG_W) ends_out[(long long)b * N_max + n] = n < N ? ends[n] : Tb;
    if (path)
        for (int t = l; t < T; t += RG_W) {
            int lo = -1;
            if (t < Tb) {                                                   // the smallest n < N with ends[n] > t; ends[N - 1] >= Tb > t
                lo = 0;
                int hi = N - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ends[mid] > t) hi = mid;
                    else lo = mid + 1;
                }
            }
            path[(long long)b * T + t] = lo;
        }
}

// grid (ceil(T / frames), B): the workgroup's frames t0 .. t0 + frames - 1, `cw` groups of four channels (vec) or channels a row
template <bool VEC>
__global__ void __launch_bounds__(RG_W) regulate_expand_kernel(const float* __restrict__ x, long long xb, long long xn,
                                                               const int* __restrict__ path, int T, int C, int cw, int frames,
                                                               float* __restrict__ y) {
    const int b = blockIdx.y, t0 = blockIdx.x * frames;
    const int rows = T - t0 < frames ? T - t0 : frames;
    const float* xu = x + b * xb;
    const int* pu = path + (long long)b * T;
    float* yu = y + (long long)b * T * C;
    for (int i = threadIdx.x; i < rows * cw; i += RG_W) {
        const int t = t0 + i / cw, c = i % cw;
        const int n = pu[t];
        if (VEC) {
            const float4 v = n >= 0 ? t2_ld4(xu + n * xn + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
            t2_st4(yu + (long long)t * C + 4 * c, v);
        } else {
            yu[(long long)t * C + c] = n >= 0 ? xu[n * xn + c] : 0.0f;
        }
    }
}

// grid (ceil(N_max / (RG_W / width)), B): `width` lanes a token
__global__ void __launch_bounds__(RG_W) regulate_segsum_kernel(const float* __restrict__ dy, long long gb, long long gt,
                                                               const int* __restrict__ ends, int N_max, int C, int width,
                                                               float* __restrict__ dx) {
    const int b = blockIdx.y, n = blockIdx.x * (RG_W / width) + threadIdx.x / width, c0 = threadIdx.x % width;
    if (n >= N_max) return;
    const int* e = ends + (long long)b * N_max;
    const int t0 = n > 0 ? e[n - 1] : 0, t1 = e[n];
    const float* g = dy + b * gb;
    for (int c = c0; c < C; c += width) {
        float s = 0.0f;
        if (t0 < t1) {
            s = g[t0 * gt + c];
            for (int t = t0 + 1; t < t1; ++t) s += g[t * gt + c];
        }
        dx[((long long)b * N_max + n) * C + c] = s;
    }
}

// the same grid; num (NULL: not wanted) and m (B, N_max, C), den (B, N_max)
__global__ void __launch_bounds__(RG_W) regulate_pool_kernel(const float* __restrict__ v, long long vb, long long vt,
                                                             const float* __restrict__ w, long long wb,
                                                             const int* __restrict__ ends, int N_max, int C, int width,
                                                             float* __restrict__ m, float* __restrict__ den,
                                                             float* __restrict__ num) {
    const int b = blockIdx.y, n = blockIdx.x * (RG_W / width) + threadIdx.x / width, c0 = threadIdx.x % width;
    if (n >= N_max) return;
    const int* e = ends + (long long)b * N_max;
    const int t0 = n > 0 ? e[n - 1] : 0, t1 = e[n];
    const float* vu = v + b * vb;
    const float* wu = w ? w + b * wb : nullptr;
    float dn = 0.0f;
    for (int t = t0; t < t1; ++t) dn += wu ? wu[t] : 1.0f;
    if (c0 == 0) den[(long long)b * N_max + n] = dn;
    for (int c = c0; c < C; c += width) {
        float s = 0.0f;
        for (int t = t0; t < t1; ++t) s = fmaf(wu ? wu[t] : 1.0f, vu[t * vt + c], s);
        const long long o = ((long long)b * N_max + n) * C + c;
        if (num) num[o] = s;
        m[o] = dn > 0.0f ? s / dn : 0.0f;
    }
}

// grid (ceil(T / frames), B): dv (B, T, C)
__global__ void __launch_bounds__(RG_W) regulate_pool_bwd_kernel(const float* __restrict__ g, const float* __restrict__ den,
                                                                 const float* __restrict__ w, long long wb,
                                                                 const int* __restrict__ path, int T, int N_max, int C, int frames,
                                                                 float* __restrict__ dv) {
    const int b = blockIdx.y, t0 = blockIdx.x * frames;
    const int rows = T - t0 < frames ? T - t0 : frames;
    const int* pu = path + (long long)b * T;
    for (int i = threadIdx.x; i < rows * C; i += RG_W) {
        const int t = t0 + i / C, c = i % C;
        const int n = pu[t];
        float r = 0.0f;
        if (n >= 0) {
            const float dn = den[(long long)b * N_max + n];
            if (dn > 0.0f) r = (w ? w[b * wb + t] : 1.0f) * (g[((long long)b * N_max + n) * C + c] / dn);
        }
        dv[((long long)b * T + t) * C + c] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static int rg_check(const char* who, int B, int N_max, int T, int C, int t_min) {
    char msg[160];
    const char* what = !(B >= 1 && B <= RG_MAX_B)   ? "1 to 65535 utterances"
                       : !(N_max >= 1)              ? "at least 1 token"
                       : !(N_max <= RG_MAX_N)       ? "at most 1024 tokens"
                       : !(T >= t_min)              ? (t_min ? "at least 1 frame" : "a frame count of at least 0")
                       : !(T <= RG_MAX_T)           ? "at most 65536 frames"
                       : !(C >= 1 && C <= RG_MAX_C) ? "1 to 512 channels"
                                                    : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, sizeof(msg), "%s: %s: B %d tokens %d frames %d channels %d", who, what, B, N_max, T, C);
    T2_FAIL(msg);
}

static inline int rg_width(int C) {
    int w = 1;
    while (w < C && w < 64) w <<= 1;
    return w;
}

extern "C" int t2amd_regulate_limits(int* max_channels, int* max_tokens, int* max_frames) {
    T2_REQUIRE(max_channels && max_tokens && max_frames, "regulate_limits: null operand");
    *max_channels = RG_MAX_C;
    *max_tokens = RG_MAX_N;
    *max_frames = RG_MAX_T;
    return T2AMD_OK;
}

extern "C" int t2amd_durations_to_path_i32(const void* durations, int duration_bytes, long long db, const int* n_len, int B,
                                           int N_max, int T, int* path, int* t_lengths, int* ends, long long* totals,
                                           void* stream) {
    T2_REQUIRE(durations && t_lengths, "durations_to_path: null operand");
    T2_PROPAGATE(rg_check("durations_to_path", B, N_max, T, 1, 0));
    T2_REQUIRE(duration_bytes == 4 || duration_bytes == 8, "durations_to_path: durations are int32 (4) or int64 (8)");
    T2_REQUIRE(db >= N_max || B == 1, "durations_to_path: the duration stride is shorter than a row");
    const long long dbytes = duration_bytes * ((B - 1) * db + N_max);
    T2_REQUIRE(!(path && t2_overlap(path, 4LL * B * T, durations, dbytes)) && !t2_overlap(t_lengths, 4LL * B, durations, dbytes) &&
                   !(ends && t2_overlap(ends, 4LL * B * N_max, durations, dbytes)) &&
                   !(totals && t2_overlap(totals, 8LL * B, durations, dbytes)),
               "durations_to_path: outputs must not overlap the durations");
    if (duration_bytes == 4)
        T2_LAUNCH(regulate_path_kernel<int>, dim3((unsigned)B), dim3(RG_W), 0, (hipStream_t)stream, (const int*)durations, db, n_len,
                  N_max, T, path, t_lengths, ends, totals);
    else
        T2_LAUNCH(regulate_path_kernel<long long>, dim3((unsigned)B), dim3(RG_W), 0, (hipStream_t)stream,
                  (const long long*)durations, db, n_len, N_max, T, path, t_lengths, ends, totals);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_length_regulate_f32(const float* x, long long xb, long long xn, const int* path, int B, int N_max, int T, int C,
                                         float* y, void* stream) {
    T2_REQUIRE(x && path && y, "length_regulate: null operand");
    T2_PROPAGATE(rg_check("length_regulate", B, N_max, T, C, 1));
    T2_REQUIRE(t2_strides_cover(xb, xn, B, N_max, C), "length_regulate: token strides shorter than the rows");
    T2_REQUIRE(!t2_overlap(y, 4LL * B * T * C, x, t2_span_bytes(xb, xn, B, N_max, C)) && !t2_overlap(y, 4LL * B * T * C, path, 4LL * B * T),
               "length_regulate: the output must not overlap the inputs");
    const bool vec = (C & 3) == 0 && t2_aligned16(x) && t2_aligned16(y) && (xn & 3) == 0 && (B == 1 || (xb & 3) == 0);
    const int cw = vec ? C / 4 : C, frames = RG_ITEMS / cw > 1 ? RG_ITEMS / cw : 1;
    const dim3 grid((unsigned)t2_cdiv(T, frames), (unsigned)B);
    if (vec)
        T2_LAUNCH(regulate_expand_kernel<true>, grid, dim3(RG_W), 0, (hipStream_t)stream, x, xb, xn, path, T, C, cw, frames, y);
    else
        T2_LAUNCH(regulate_expand_kernel<false>, grid, dim3(RG_W), 0, (hipStream_t)stream, x, xb, xn, path, T, C, cw, frames, y);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_length_regulate_bwd_f32(const float* dy, long long gb, long long gt, const int* ends, int B, int N_max, int T,
                                             int C, float* dx, void* stream) {
    T2_REQUIRE(dy && ends && dx, "length_regulate_bwd: null operand");
    T2_PROPAGATE(rg_check("length_regulate_bwd", B, N_max, T, C, 1));
    T2_REQUIRE(t2_strides_cover(gb, gt, B, T, C), "length_regulate_bwd: gradient strides shorter than the rows");
    T2_REQUIRE(!t2_overlap(dx, 4LL * B * N_max * C, dy, t2_span_bytes(gb, gt, B, T, C)) &&
                   !t2_overlap(dx, 4LL * B * N_max * C, ends, 4LL * B * N_max),
               "length_regulate_bwd: the output must not overlap the inputs");
    const int width = rg_width(C);
    T2_LAUNCH(regulate_segsum_kernel, dim3((unsigned)t2_cdiv(N_max, RG_W / width), (unsigned)B), dim3(RG_W), 0, (hipStream_t)stream,
              dy, gb, gt, ends, N_max, C, width, dx);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_token_average_f32(const float* v, long long vb, long long vt, const float* w, long long wb, const int* ends,
                                       int B, int N_max, int T, int C, float* m, float* den, float* num, void* stream) {
    T2_REQUIRE(v && ends && m && den, "token_average: null operand");
    T2_PROPAGATE(rg_check("token_average", B, N_max, T, C, 1));
    T2_REQUIRE(t2_strides_cover(vb, vt, B, T, C), "token_average: value strides shorter than the rows");
    T2_REQUIRE(!w || B == 1 || wb >= T, "token_average: the weight stride is shorter than a row");
    const long long vbytes = t2_span_bytes(vb, vt, B, T, C), wbytes = 4 * ((B - 1) * wb + T), obytes = 4LL * B * N_max * C;
    T2_REQUIRE(!t2_overlap(m, obytes, v, vbytes) && !t2_overlap(den, 4LL * B * N_max, v, vbytes) &&
                   !t2_overlap(m, obytes, ends, 4LL * B * N_max) && !t2_overlap(den, 4LL * B * N_max, ends, 4LL * B * N_max) &&
                   !t2_overlap(m, obytes, den, 4LL * B * N_max) &&
                   !(w && (t2_overlap(m, obytes, w, wbytes) || t2_overlap(den, 4LL * B * N_max, w, wbytes))) &&
                   !(num && (t2_overlap(num, obytes, v, vbytes) || t2_overlap(num, obytes, m, obytes) ||
                             t2_overlap(num, obytes, den, 4LL * B * N_max) || t2_overlap(num, obytes, ends, 4LL * B * N_max) ||
                             (w && t2_overlap(num, obytes, w, wbytes)))),
               "token_average: outputs must not overlap the inputs or each other");
    const int width = rg_width(C);
    T2_LAUNCH(regulate_pool_kernel, dim3((unsigned)t2_cdiv(N_max, RG_W / width), (unsigned)B), dim3(RG_W), 0, (hipStream_t)stream, v,
              vb, vt, w, wb, ends, N_max, C, width, m, den, num);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}

extern "C" int t2amd_token_average_bwd_f32(const float* g, const float* den, const float* w, long long wb, const int* path, int B,
                                           int N_max, int T, int C, float* dv, void* stream) {
    T2_REQUIRE(g && den && path && dv, "token_average_bwd: null operand");
    T2_PROPAGATE(rg_check("token_average_bwd", B, N_max, T, C, 1));
    T2_REQUIRE(!w || B == 1 || wb >= T, "token_average_bwd: the weight stride is shorter than a row");
    const long long obytes = 4LL * B * T * C;
    T2_REQUIRE(!t2_overlap(dv, obytes, g, 4LL * B * N_max * C) && !t2_overlap(dv, obytes, den, 4LL * B * N_max) &&
                   !t2_overlap(dv, obytes, path, 4LL * B * T) && !(w && t2_overlap(dv, obytes, w, 4 * ((B - 1) * wb + T))),
               "token_average_bwd: the output must not overlap the inputs");
    const int frames = RG_ITEMS / C > 1 ? RG_ITEMS / C : 1;
    T2_LAUNCH(regulate_pool_bwd_kernel, dim3((unsigned)t2_cdiv(T, frames), (unsigned)B), dim3(RG_W), 0, (hipStream_t)stream, g, den, w,
              wb, path, T, N_max, C, frames, dv);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
