// Shared device/host helpers for the MI355X (gfx950 / CDNA4) Tacotron 2 mel engine.
// Wave = 64 lanes everywhere; MFMA f32 forms are exact-f32 (k-ordered fmaf chain).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/tacotron2_amd.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define T2_WAVE 64

// Last error text, readable through t2amd_last_error().
extern "C" void t2amd_set_error_(const char* msg);

#define T2_FAIL(msg)                                                                   \
    do {                                                                               \
        t2amd_set_error_(msg);                                                         \
        return T2AMD_ERR_ARG;                                                          \
    } while (0)

#define T2_REQUIRE(cond, msg)                                                          \
    do {                                                                               \
        if (!(cond)) T2_FAIL(msg);                                                     \
    } while (0)

// Validate-only mode (t2amd_set_validate_only): every host-side check and loop runs, no kernel is
// launched.  Used by the CPU test-suite to exercise argument plumbing without a GPU; outputs are
// left untouched, so it is NOT a compute path.
extern "C" int t2amd_validate_only_flag_(void);

extern "C" void t2amd_profile_mark_(int tag, int end, hipStream_t s);

#define T2_LAUNCH(kern, grid, block, lds, stream, ...)                                 \
    do {                                                                               \
        if (!t2amd_validate_only_flag_())                                              \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);           \
    } while (0)

// The same launch carrying an event pair when bench.py's roofline leg profiles role `role` (t2amd_profile_enable): the
// pair is stamped by the dispatch itself (hipExtLaunchKernelGGL start/stop events = the kernel begin/end timestamps
// rocprofv3 --kernel-trace reports), so there is no bracket overhead to calibrate away.  Roles: 3 fused LSTM pair of a
// decoder time step, 4 attention backward (+ folded cells), 5 attention forward (one-launch form), 6 BPTT dgrad pair,
// 7 the persistent forward loop (all time steps' LSTM pairs and attention steps in ONE launch).
extern "C" bool t2amd_profile_pair_(int tag, hipEvent_t* e0, hipEvent_t* e1);
#define T2_LAUNCH_ROLE(role, kern, grid, block, lds, stream, ...)                      \
    do {                                                                               \
        if (t2amd_validate_only_flag_()) break;                                        \
        hipEvent_t pe0_ = nullptr, pe1_ = nullptr;                                     \
        if (t2amd_profile_pair_(role, &pe0_, &pe1_))                                   \
            hipExtLaunchKernelGGL(kern, grid, block, lds, stream, pe0_, pe1_, 0, __VA_ARGS__); \
        else                                                                           \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);           \
    } while (0)

#define T2_LAUNCH_CHECK()                                                              \
    do {                                                                               \
        if (t2amd_validate_only_flag_()) break;                                        \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess) {                                                        \
            t2amd_set_error_(hipGetErrorString(e_));                                   \
            return T2AMD_ERR_LAUNCH;                                                   \
        }                                                                              \
    } while (0)

#define T2_PROPAGATE(call)                                                             \
    do {                                                                               \
        int rc_ = (call);                                                              \
        if (rc_ != T2AMD_OK) return rc_;                                               \
    } while (0)

// f32 -> bf16 bits, round to nearest even
__device__ __forceinline__ unsigned short t2_f32_to_bf16(float x) {
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// two f32 -> packed bf16 pair (a in the low half), round to nearest even, one VALU instruction
__device__ __forceinline__ unsigned t2_cvt_pk_bf16(float a, float b) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---- split-bf16 operand images (round 6: the 'bf16x3' mode of the LSTM tiles, include/tacotron2_amd.h t2amd_split_bf16x3_f32) ----
// x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in f32): 16 mantissa bits, |x - hi - lo| <= 2^-17 |x|.
__device__ __forceinline__ void t2_split_bf16(float x, unsigned short& hi, unsigned short& lo) {
    hi = t2_f32_to_bf16(x);
    lo = t2_f32_to_bf16(x - __uint_as_float((unsigned)hi << 16));
}
// position (in bf16 units) of k's hi value inside a row of the split image: groups of 16 k = 16 hi then 16 lo; lo sits 16 further
__device__ __forceinline__ long long t2_x3_pos(long long k) { return ((k >> 4) << 5) + (k & 15); }

__device__ __forceinline__ float t2_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// sigmoid on v_exp_f32 / v_rcp_f32 (|err| ~1e-7): the bf16-mode kernels' cell; the parity-mode kernels keep libm's
__device__ __forceinline__ float t2_sigmoid_fast(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}
// tanh without divergent paths (libm's tanhf is two exec-masked branches, both taken by a mixed wave).
// |x| < 0.625: x + x*x2*P(x2), the minimax polynomial libm uses on that range; otherwise 1 - 2/(exp(2|x|) + 1) on
// v_exp_f32 / v_rcp_f32 (absolute error < 5e-7).  Both are evaluated and one is selected.
__device__ __forceinline__ float t2_tanh(float x) {
    const float ax = fabsf(x);
    const float x2 = ax * ax;
    float p = fmaf(x2, __uint_as_float(0xbbbac73du), __uint_as_float(0x3ca908c9u));
    p = fmaf(x2, p, __uint_as_float(0xbd5c1c4eu));
    p = fmaf(x2, p, __uint_as_float(0x3e088382u));
    p = fmaf(x2, p, __uint_as_float(0xbeaaaa99u));
    const float small = fmaf(x2, ax * p, ax);
    const float e = __builtin_amdgcn_exp2f(ax * 2.8853900817779268f);      // exp(2|x|); inf for large |x| -> big = 1
    const float big = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
    return copysignf(ax < 0.625f ? small : big, x);
}

// One-range form for the bf16 compute mode of the TRAINING loops (round 5): tanh(x) = 1 - 2 / (exp(2x) + 1) straight on v_exp_f32 /
// v_rcp_f32 -- 5 VALU operations instead of ~17 (no |x|, no polynomial, no select, no copysign); exp -> inf gives 1, exp -> 0 gives -1.
// Absolute error < 3e-7 like the two-range form's large branch, but NOT relatively accurate near 0 (|x| < 1e-3: the subtraction loses
// it): fine beside bf16 products (the attention energies sum v * tanh), not for the fp32 parity mode, which keeps t2_tanh.  The
// attention backward recomputes the forward's tanh with the same selection, so the pair stays consistent.  -DT2AMD_TANH_EXACT: off.
__device__ __forceinline__ float t2_tanh_1r(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}
template <bool FAST>
__device__ __forceinline__ float t2_tanh_sel(float x) {
#ifdef T2AMD_TANH_EXACT
    return t2_tanh(x);
#else
    if constexpr (FAST) return t2_tanh_1r(x);
    else return t2_tanh(x);
#endif
}

// DPP lane exchanges (VALU, no LDS crossbar: a __shfl_xor is a ds_bpermute the compiler waits for one at a time).
// The four steps pair exactly the lanes the xor-1/2/4/8 butterfly pairs, so sums are bitwise the same.
template <int CTRL>
__device__ __forceinline__ float t2_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sum over each aligned group of 16 lanes, result in every lane of the group
__device__ __forceinline__ float row16_sum(float v) {
    v += t2_dpp<0xB1>(v);      // quad_perm [1,0,3,2]  (lane ^ 1)
    v += t2_dpp<0x4E>(v);      // quad_perm [2,3,0,1]  (lane ^ 2)
    v += t2_dpp<0x141>(v);     // row_half_mirror      (the other quad of the 8-lane half: same partner sums as lane ^ 4)
    v += t2_dpp<0x140>(v);     // row_mirror           (the other half of the row: as lane ^ 8)
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, t2_dpp<0xB1>(v));
    v = fmaxf(v, t2_dpp<0x4E>(v));
    v = fmaxf(v, t2_dpp<0x141>(v));
    v = fmaxf(v, t2_dpp<0x140>(v));
    return v;
}
__device__ __forceinline__ float wave_reduce_sum(float v) {
    v = row16_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float wave_reduce_max(float v) {
    v = row16_max(v);
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}


// tools only: phase stamps of ONE mid-loop launch per instrumented kernel.  Compiled in only with
// -DT2AMD_PHASE_STAMPS (python -m tacotron2_amd.build --stamps -> lib/libtacotron2_amd_stamps.so, selected with
// T2AMD_LIB) -- even a never-taken stamp branch in the chain kernels costs ~2 % of a training step.  With
// T2AMD_ATTN_TS=1, thread 0 of workgroup 0 counts the launches of its kernel in slot base+15 and stamps only the launch
// whose number is in slot 127 (T2AMD_ATTN_TS_PICK, default 1200 = second training step, mid sequence), so that
// tools/phase_stamps_step.py sees a warm, regular step rather than the last (special) one.
__device__ __forceinline__ bool t2_ts_begin(unsigned long long* ts, int base) {
    if (!ts || blockIdx.x != 0 || blockIdx.y != 0 || threadIdx.x != 0) return false;
    const unsigned long long n = atomicAdd(&ts[base + 15], 1ull);
    if (n != ts[127]) return false;
    ts[base] = wall_clock64();
    return true;
}
__device__ __forceinline__ void t2_ts_mark(bool on, unsigned long long* ts, int slot) {
    if (on) ts[slot] = wall_clock64();
}

// internal entry points shared between translation units (not part of the C ABI)
extern "C" unsigned long long* t2amd_debug_ts_();
int t2amd_proj_finish_small_(const t2amd_small_linear* a, int* out_lengths, uint8_t* active, int* done_count, int t,
                             int max_steps, float thr, int gate_row, void* stream);

int t2amd_check_lstm_bwd_(const t2amd_lstm_bwd* a);      // rnn.hip: argument checks of one cell-backward descriptor

static inline bool t2_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int t2_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline long long t2_round_up(long long n, long long m) { return (n + m - 1) / m * m; }

// A padded batch of B matrices of `rows` rows of `cols` floats, batch stride bs and row stride ld (in floats): do the strides
// cover the matrix, and the bytes from its first float to its last.  The checks of the alignment, aligner, regulator,
// self-attention and FFT-block entries.
static inline bool t2_strides_cover(long long bs, long long ld, int B, int rows, long long cols) {
    return ld >= cols && (B == 1 || bs >= (long long)(rows - 1) * ld + cols);
}
static inline long long t2_span_bytes(long long bs, long long ld, int B, int rows, long long cols) {
    return 4 * ((B - 1) * bs + (long long)(rows - 1) * ld + cols);
}

// index into y[0..T) of padded sample i (i already shifted by -pad): torch 'reflect' (edge sample not repeated).  The one
// statement of the mirror rule: the forward pad (audio.hip) and the gradient's fold (audio_bwd.hip) both call it.
static __host__ __device__ __forceinline__ long long t2_reflect(long long i, long long T) {
    if (i < 0) i = -i;
    if (i >= T) i = 2 * (T - 1) - i;
    return i;
}

// The most rows of a packed row image (HiFi-GAN, Vocos): 2^31 - 256, so that grid.x = rows / 128 and 32-bit row sums hold
#define T2_MAX_ROWS 2147483392LL

// ---- row-kernel helpers of the audio losses and the vocoders ------------------------------------------------------------------
// Plain C++ and __shfl_xor only (no DPP, no builtins): tests/hip_emu compiles them with the kernels that call them.  Each is the
// one statement of something a backward kernel must repeat bit for bit from its forward, or of a layout two kernels share.

// re^2 + im^2 of a spectrum bin, three roundings: the magnitude of audio.hip and vocoder.hip, recomputed by audio_bwd.hip and
// stft_loss.hip ("the forward's bits")
__device__ __forceinline__ float t2_power(float re, float im) { return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)); }

// sum over the wave as a xor butterfly 32, 16, .. 1: the same bits in every lane.  NOT wave_reduce_sum: its DPP steps associate
// in another order.  (float clients only so far: on the float64 sums below it moved instructions.)
template <class T>
__device__ __forceinline__ T t2_wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// The fixed-order float64 sum of a 256-thread workgroup (stft_loss_fwd_kernel, stft_loss_finish_kernel, mel_l1_fwd_kernel): the
// xor butterfly in every wave, the four wave sums into LDS, a barrier, then this combine in thread 0.  The first three steps stay
// written out in the kernels: as a helper they made the compiler schedule those kernels differently.
__device__ __forceinline__ double t2_block_total_f64(const double (&w)[4]) { return ((w[0] + w[1]) + w[2]) + w[3]; }

// a per-utterance count clamped into [0, n]
__device__ __forceinline__ int t2_clamp_count(int c, int n) {
    if (c > n) c = n;
    return c < 0 ? 0 : c;
}

__device__ __forceinline__ float4 t2_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void t2_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// The d_spec row of the spectral backward, [d_re (F) | d_im (F) | 0 (Kp - 2F)]: spec's own column layout at the row stride the
// product d_frames = d_spec . forward_basis wants.  The lane of bin f stores its two values and the padding columns 2F + f,
// 3F + f, ... below Kp; row0 = the row's first float.  Written by magnitude_bwd_kernel (audio_bwd.hip) and stft_loss_bwd_kernel (stft_loss.hip), one lane per
// bin, rows * F lanes in workgroups of 256.
__device__ __forceinline__ void t2_dspec_store(float* d_spec, long long row0, int f, int F, int Kp, float dre, float dim) {
    d_spec[row0 + f] = dre;
    d_spec[row0 + F + f] = dim;
    for (int c = 2 * F + f; c < Kp; c += F) d_spec[row0 + c] = 0.0f;
}

// host side of the same: the checks of Kp and ldd and the workgroups of a launch over rows * F lanes (rows > 0 and
// 0 < F <= 65536 already checked); `who` is the entry point's prefix of the error text
static inline int t2_dspec_blocks(const char* who, long long rows, int F, int Kp, long long ldd, unsigned* blocks) {
    char msg[160];
    const long long nb = (rows * F + 255) / 256;
    const char* what = !(Kp >= 2 * F && Kp <= 2 * F + 65536) ? "d_spec rows hold 2 F values and the padding columns"
                       : ldd < Kp                            ? "row too short"
                       : nb > 0x7fffffffLL                   ? "too many elements for one launch"
                                                             : nullptr;
    if (what) {
        snprintf(msg, sizeof(msg), "%s: %s", who, what);
        T2_FAIL(msg);
    }
    *blocks = (unsigned)nb;
    return T2AMD_OK;
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte: the aliasing check of an output against an input
static inline bool t2_overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)b_bytes && pb < pa + (uintptr_t)a_bytes;
}
