// F0 extraction by YIN (tacotron2_amd/audio.py yin; de Cheveigne and Kawahara 2002).
//   frame t of an utterance of n samples is x[t hop - L/2 : t hop + L/2] with zeros outside [0, n); there are n / hop + 1 of them
//   (the mel front end's count: F0 frame t and mel column t share the centre sample t hop).  With W = L / 2:
//   d(tau)  = sum_{j<W} (f[j] - f[j+tau])^2, tau = 1 .. tau_max + 1: the difference first, ascending j, one fma each;
//   d'(0)   = 1, d'(tau) = d(tau) tau / S(tau), S(tau) = d(1) + .. + d(tau), and 1 where S(tau) == 0;
//   lag     = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, d'(tau) < d'(tau-1), d'(tau) <= d'(tau+1) (voiced),
//             else the argmin of d' over the range, smallest lag on ties (unvoiced);
//   shift   = -b / a, a = d'(tau-1) + d'(tau+1) - 2 d'(tau), b = (d'(tau+1) - d'(tau-1)) / 2, where a > 0 and |b| <= a / 2, else 0;
//             |b| <= a / 2 is d'(tau) <= min(d'(tau-1), d'(tau+1)) and is tested in that form, by comparisons alone;
//   f0 = sr / (tau + shift), voiced, aperiodicity = d'(tau).  Frames at and beyond the count get 0 / 0 / 0.
// Layout: one workgroup of 256 lanes per frame.  The frame is staged in LDS once (16-byte loads of whole aligned groups inside
// the signal, the zeros written explicitly).  Lanes own lags: lane l does tau = l + 1 and l + 257 together, then + 512 ...; f[j..j+3]
// is one 16-byte broadcast read per four j, f[j + tau] is consecutive across lanes.  S is a fixed-order workgroup prefix sum: each
// lane sums its own run of consecutive lags, a Hillis-Steele scan links the 256 runs.  The choice of lag is one 64-bit
// min-reduction: a qualifying lag is its own key, every other lag of the range is 2^63 + d' bits 2^32 + tau (d' >= 0, so its
// bits order as it does).  Lane 0 refines and stores.  One writer per element, fixed order, no atomics: two calls give the same
// bits, a frame does not depend on its batch, and the optional slab of d' changes nothing.  Plain C++, __syncthreads and
// __shfl_xor only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define YIN_THREADS 256
#define YIN_MAX_L 4096                  /* frame_length at most: 16 KiB of LDS for the frame, 8 KiB for d' */
#define YIN_SMALL_L 1024                /* the instantiation the default geometry takes: 4 + 2 KiB, more workgroups per CU */

// d(ta) and d(tb) together: two independent accumulators behind one broadcast read of f[j .. j+3]
__device__ __forceinline__ void yin_diff2(const float* __restrict__ f, int W, int ta, int tb, float& da, float& db) {
    const float *fa = f + ta, *fb = f + tb;
    float acca = 0.0f, accb = 0.0f;
    int j = 0;
    for (; j + 4 <= W; j += 4) {
        const float4 c = t2_ld4(f + j);
        float u;
        u = c.x - fa[j];
        acca = fmaf(u, u, acca);
        u = c.x - fb[j];
        accb = fmaf(u, u, accb);
        u = c.y - fa[j + 1];
        acca = fmaf(u, u, acca);
        u = c.y - fb[j + 1];
        accb = fmaf(u, u, accb);
        u = c.z - fa[j + 2];
        acca = fmaf(u, u, acca);
        u = c.z - fb[j + 2];
        accb = fmaf(u, u, accb);
        u = c.w - fa[j + 3];
        acca = fmaf(u, u, acca);
        u = c.w - fb[j + 3];
        accb = fmaf(u, u, accb);
    }
    for (; j < W; ++j) {
        float u = f[j] - fa[j];
        acca = fmaf(u, u, acca);
        u = f[j] - fb[j];
        accb = fmaf(u, u, accb);
    }
    da = acca;
    db = accb;
}

__device__ __forceinline__ float yin_diff1(const float* __restrict__ f, int W, int ta) {
    const float* fa = f + ta;
    float acc = 0.0f;
    int j = 0;
    for (; j + 4 <= W; j += 4) {
        const float4 c = t2_ld4(f + j);
        float u;
        u = c.x - fa[j];
        acc = fmaf(u, u, acc);
        u = c.y - fa[j + 1];
        acc = fmaf(u, u, acc);
        u = c.z - fa[j + 2];
        acc = fmaf(u, u, acc);
        u = c.w - fa[j + 3];
        acc = fmaf(u, u, acc);
    }
    for (; j < W; ++j) {
        const float u = f[j] - fa[j];
        acc = fmaf(u, u, acc);
    }
    return acc;
}

template <int ML>
__global__ void __launch_bounds__(YIN_THREADS) yin_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lengths,
                                                          long long T, int frames, int L, int hop, int tau_min, int tau_max,
                                                          float sr, float threshold, float* __restrict__ f0,
                                                          unsigned char* __restrict__ voiced, float* __restrict__ aperiodicity,
                                                          float* __restrict__ dprime) {
    __shared__ __attribute__((aligned(16))) float f[ML];
    __shared__ float d[ML / 2 + 2];                                         // d(tau), then d'(tau), tau = 0 .. tau_max + 1
    __shared__ float sc[2][YIN_THREADS];
    __shared__ unsigned long long wk[YIN_THREADS / T2_WAVE];
    const int t = blockIdx.x, b = blockIdx.y, l = threadIdx.x;
    const int W = L / 2, nl = tau_max + 1;                                  // lags 1 .. nl; W + nl <= L <= ML (the host checks)
    long long n = lengths ? (long long)lengths[b] : T;
    n = n > T ? T : n;
    const long long count = n < 1 ? 0 : n / hop + 1;                        // the host refuses lengths below 1
    const long long row = (long long)b * frames + t;
    if (t >= count) {                                                       // uniform over the workgroup
        if (l == 0) {
            f0[row] = 0.0f;
            voiced[row] = 0;
            aperiodicity[row] = 0.0f;
        }
        if (dprime)
            for (int i = l; i <= nl; i += YIN_THREADS) dprime[row * (nl + 1) + i] = 0.0f;
        return;
    }

    // ---- the frame into LDS: whole 16-byte groups of memory, one load each where the group lies inside the frame and the signal
    const float* xb = x + b * ldx;
    const long long s0 = (long long)t * hop - W;                            // the sample of f[0]
    const int mis = (int)(((unsigned long long)(reinterpret_cast<uintptr_t>(xb) >> 2) + (unsigned long long)s0) & 3ull);
    const int ngroups = (L + mis + 3) / 4;
    for (int g = l; g < ngroups; g += YIN_THREADS) {
        const int i0 = 4 * g - mis;                                         // f index of the group's first float (< 0: before the frame)
        const long long s = s0 + i0;                                        // its sample: xb + s is 16-byte aligned
        if (i0 >= 0 && i0 + 4 <= L && s >= 0 && s + 4 <= n) {
            const float4 v = t2_ld4(xb + s);
            f[i0] = v.x;
            f[i0 + 1] = v.y;
            f[i0 + 2] = v.z;
            f[i0 + 3] = v.w;
        } else {
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + e;
                const long long q = s + e;
                if (i >= 0 && i < L) f[i] = q >= 0 && q < n ? xb[q] : 0.0f;
            }
        }
    }
    if (l == 0) d[0] = 1.0f;
    __syncthreads();

    // ---- d(tau): lanes own lags, two at a time
    for (int base = 0; base < nl; base += 2 * YIN_THREADS) {
        const int ta = base + l + 1, tb = ta + YIN_THREADS;
        const int wave_first = ta - (l & (T2_WAVE - 1));                    // the wave's first lag: what follows is uniform over it
        if (wave_first + YIN_THREADS <= nl) {
            float da, db;
            yin_diff2(f, W, ta <= nl ? ta : 1, tb <= nl ? tb : 1, da, db);  // a lane without a lag computes d(1) and drops it
            if (ta <= nl) d[ta] = da;
            if (tb <= nl) d[tb] = db;
        } else if (wave_first <= nl) {
            const float da = yin_diff1(f, W, ta <= nl ? ta : 1);
            if (ta <= nl) d[ta] = da;
        }
    }
    __syncthreads();

    // ---- S(tau) and d'(tau): lane l owns the run of C consecutive lags l C + 1 .. (l + 1) C
    const int C = (nl + YIN_THREADS - 1) / YIN_THREADS;
    const int first = l * C + 1, last = first + C - 1 < nl ? first + C - 1 : nl;
    float run = 0.0f;
    for (int tau = first; tau <= last; ++tau) run += d[tau];
    sc[0][l] = run;
    __syncthreads();
    int cur = 0;
    for (int s = 1; s < YIN_THREADS; s <<= 1) {
        const float v = l >= s ? sc[cur][l - s] + sc[cur][l] : sc[cur][l];
        sc[cur ^ 1][l] = v;
        cur ^= 1;
        __syncthreads();
    }
    run = l > 0 ? sc[cur][l - 1] : 0.0f;
    for (int tau = first; tau <= last; ++tau) {
        const float v = d[tau];
        run += v;
        d[tau] = run > 0.0f ? v * (float)tau / run : 1.0f;
    }
    __syncthreads();

    // ---- the choice of lag: one min over 64-bit keys
    unsigned long long key = ~0ull;
    for (int tau = tau_min + l; tau <= tau_max; tau += YIN_THREADS) {
        const float v = d[tau];
        const bool dip = v < threshold && v < d[tau - 1] && v <= d[tau + 1];
        const unsigned long long k = dip ? (unsigned long long)tau
                                         : (1ull << 63) | ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)tau;
        key = k < key ? k : key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
    }
    if ((l & (T2_WAVE - 1)) == 0) wk[l / T2_WAVE] = key;
    __syncthreads();
    if (l == 0) {
        for (int w = 1; w < YIN_THREADS / T2_WAVE; ++w) key = wk[w] < key ? wk[w] : key;
        const bool isv = (key >> 63) == 0;
        int tau = (int)(key & 0xffffffffull);
        if (tau < tau_min || tau > tau_max) tau = tau_min;                  // every d' a NaN: nothing compared below anything
        const float dm = d[tau - 1], d0 = d[tau], dp = d[tau + 1];
        float shift = 0.0f;
        if (d0 <= dm && d0 <= dp) {                                         // |b| <= a / 2, exactly
            const float a = (dm + dp) - 2.0f * d0, bb = (dp - dm) * 0.5f;
            if (a > 0.0f) {
                shift = -bb / a;
                shift = shift > 0.5f ? 0.5f : (shift < -0.5f ? -0.5f : shift);
            }
        }
        f0[row] = sr / ((float)tau + shift);
        voiced[row] = isv ? 1 : 0;
        aperiodicity[row] = d0;
    }
    if (dprime)
        for (int i = l; i <= nl; i += YIN_THREADS) dprime[row * (nl + 1) + i] = d[i];
}

static int yin_check(int L, int hop, int tau_min, int tau_max, char* msg) {
    const char* what = !(L >= 2 && L % 2 == 0)         ? "frame_length must be even and at least 2"
                       : !(L <= YIN_MAX_L)             ? "frame_length must not exceed 4096"
                       : !(hop >= 1)                   ? "hop_length must be at least 1"
                       : !(tau_min >= 2)               ? "tau_min = floor(sr / fmax) must be at least 2"
                       : !(tau_min <= tau_max)         ? "tau_min must not exceed tau_max"
                       : !(L / 2 + tau_max + 1 <= L)   ? "W + tau_max + 1 exceeds frame_length (W = frame_length / 2, tau_max = ceil(sr / fmin))"
                                                       : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, 200, "yin: %s: frame_length %d hop_length %d tau_min %d tau_max %d", what, L, hop, tau_min, tau_max);
    return T2AMD_ERR_ARG;
}

extern "C" int t2amd_yin_plan(double sr, int L, int hop, double fmin, double fmax, int* tau_min, int* tau_max) {
    char msg[200];
    T2_REQUIRE(tau_min && tau_max, "yin: null operand");
    T2_REQUIRE(sr > 0.0 && sr <= 16777216.0 && fmin > 0.0 && fmax > 0.0, "yin: sr, fmin and fmax must be positive");
    T2_REQUIRE(fmin < fmax, "yin: fmin must be below fmax");
    const double lo = floor(sr / fmax), hi = ceil(sr / fmin);
    const int a = lo > 1e9 ? 1000000000 : (int)lo, b = hi > 1e9 ? 1000000000 : (int)hi;
    if (yin_check(L, hop, a, b, msg) != T2AMD_OK) T2_FAIL(msg);
    *tau_min = a;
    *tau_max = b;
    return T2AMD_OK;
}

extern "C" int t2amd_yin_f32(const float* x, long long ldx, const int* lengths, int B, long long T, int frames, int L, int hop,
                             int tau_min, int tau_max, float sr, float threshold, float* f0, unsigned char* voiced,
                             float* aperiodicity, float* dprime, void* stream) {
    char msg[200];
    T2_REQUIRE(x && f0 && voiced && aperiodicity, "yin: null operand");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0, "yin: the signal is not aligned to 4 bytes");
    if (yin_check(L, hop, tau_min, tau_max, msg) != T2AMD_OK) T2_FAIL(msg);
    T2_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= 2147483647LL, "yin: 1 to 65535 utterances of 1 to 2^31 - 1 samples");
    T2_REQUIRE((long long)frames == T / hop + 1, "yin: the outputs hold T / hop_length + 1 frames per utterance");
    T2_REQUIRE(ldx >= T || B == 1, "yin: row stride shorter than the row");
    T2_REQUIRE(sr > 0.0f, "yin: sr must be positive");
    const dim3 grid((unsigned)frames, (unsigned)B);
    if (L <= YIN_SMALL_L)
        T2_LAUNCH(yin_kernel<YIN_SMALL_L>, grid, dim3(YIN_THREADS), 0, (hipStream_t)stream, x, ldx, lengths, T, frames, L, hop,
                  tau_min, tau_max, sr, threshold, f0, voiced, aperiodicity, dprime);
    else
        T2_LAUNCH(yin_kernel<YIN_MAX_L>, grid, dim3(YIN_THREADS), 0, (hipStream_t)stream, x, ldx, lengths, T, frames, L, hop,
                  tau_min, tau_max, sr, threshold, f0, voiced, aperiodicity, dprime);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
