// Masked multi-head self-attention, the MFMA-free half (tacotron2_amd/transformer.py): the row pass of the
// backward, delta(t) = sum_d g(t, d) o(t, d), and the entries that launch nothing (limits, workspace sizes).
// A row belongs to one wave: lane l runs an fmaf chain over d = l, l + 64 (ascending), then the xor butterfly 32 .. 1 of
// t2_wave_sum, which gives every lane the same bits.  Rows at and beyond the utterance's length are not read and get +0.  One
// writer per element and a fixed order: two calls give the same bits, an utterance in a ragged batch gives the bits it gives
// alone.  Plain C++, __shfl_xor only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "self_attn.h"

// grid (ceil(T / 4), B H), 256 lanes: wave w takes row 4 blockIdx.x + w
__global__ void __launch_bounds__(256) self_attn_delta_kernel(SaOperand g, const float* __restrict__ o, const int* __restrict__ len,
                                                              int T_max, int H, int D, float* __restrict__ delta) {
    const int b = blockIdx.y / H, h = blockIdx.y % H, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = len ? t2_clamp_count(len[b], T_max) : T_max;
    const int t = blockIdx.x * 4 + wave;
    const bool row = t < T;                                                 // uniform in the wave
    float s = 0.0f;
    if (row) {
        const float* gr = g.p + b * g.sb + t * g.st + h * g.sh;
        const float* orow = o + (((long long)b * T_max + t) * H + h) * D;
        for (int d = lane; d < D; d += 64) s = fmaf(gr[d], orow[d], s);
    }
    s = t2_wave_sum(s);                                                     // every lane of the workgroup takes part
    if (t < T_max && lane == 0) delta[((long long)b * H + h) * T_max + t] = row ? s : 0.0f;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
extern "C" int t2amd_self_attn_limits(int* max_frames, int* max_heads, int* min_width, int* max_width, int* max_batch_heads) {
    T2_REQUIRE(max_frames && max_heads && min_width && max_width && max_batch_heads, "self_attn: limits: null operand");
    *max_frames = SA_MAX_T;
    *max_heads = SA_MAX_H;
    *min_width = SA_MIN_D;
    *max_width = SA_MAX_D;
    *max_batch_heads = SA_MAX_BH;
    return T2AMD_OK;
}

extern "C" int t2amd_self_attn_workspace(int B, int T, int H, int D, int which, long long* bytes) {
    T2_REQUIRE(bytes, "self_attn: workspace: null operand");
    T2_PROPAGATE(sa_check("workspace", B, T, H, D));
    T2_REQUIRE(which >= 0 && which <= 2, "self_attn: workspace: which must be 0 (forward), 1 (forward, lse kept) or 2 (backward)");
    *bytes = which == 0 ? 0 : sa_rows_bytes(B, T, H);
    return T2AMD_OK;
}

extern "C" int t2amd_self_attn_delta_f32(const float* g, long long gb, long long gt, long long gh, const float* o, const int* lengths,
                                         int B, int T, int H, int D, float* delta, void* stream) {
    T2_PROPAGATE(sa_check("delta", B, T, H, D));
    const SaOperand go = {g, gb, gt, gh};
    T2_PROPAGATE(sa_check_operand("delta", "the gradient", go));
    T2_REQUIRE(o && delta, "self_attn: delta: null operand");
    const long long dbytes = 4LL * B * H * T;
    T2_REQUIRE(!t2_overlap(delta, dbytes, g, sa_span(go, B, T, H, D)) && !t2_overlap(delta, dbytes, o, 4LL * B * T * H * D),
               "self_attn: delta: the output must not overlap the inputs");
    T2_LAUNCH(self_attn_delta_kernel, dim3((unsigned)t2_cdiv(T, 4), (unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, go, o, lengths,
              T, H, D, delta);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
