// Forced alignment: the best monotonic path through a (frames, tokens) score matrix (tacotron2_amd/alignment.py, DESIGN.md
// section 18; the "monotonic alignment search" of Glow-TTS).
//   admissible path: n(0) = 0, n(T-1) = N-1, n(t) - n(t-1) in {0, 1}; 1 <= N <= T.
//   recurrence:      Q(0,0) = l(0,0), Q(0,n>0) = -inf, Q(t,n) = l(t,n) + max(Q(t-1,n), Q(t-1,n-1)), absent predecessors -inf:
//                    one rounded float32 add per cell.
//   tie rule:        staying wins: `best = stay; if (adv > best) best = adv`, strictly.
//   backtrack:       from (T-1, N-1); on the borders the walk ignores what was stored (n = 0 stays, n = t advances), so neither
//                    the workspace's content nor a non-finite score can take it outside the matrix.
//   outputs:         durations (B, N_max) int32 (frames per token, zeros at and beyond N), score (B,) = Q(T-1, N-1), and on
//                    request path (B, T_max) int32 (the token of every frame, -1 at and beyond T).
// Layout: one workgroup of ALIGN_W lanes per utterance.  Lane l owns the C consecutive columns l C .. l C + C - 1 (C = 1 or 4),
// their Q(t-1, .) in registers.  The only value a step needs from elsewhere is Q(t-1, l C - 1), the last column of lane l - 1:
// an LDS double buffer edge[2][ALIGN_W] and one __syncthreads() per step (step t reads slot (t+1)&1, writes slot t&1).
// l(t, .) does not depend on the recurrence, and the choices (1 = advance, one byte per cell) are needed only by the backtrack.
// Neither is on a step's chain, but a global store inside a step is: __syncthreads() releases the workgroup's earlier stores, so
// the compiler puts s_waitcnt vmcnt(0) in front of the s_barrier of every step that has stored, which also waits for every load
// in flight.  So memory is touched in bursts: ALIGN_ROWS rows of l are loaded into registers at once, ALIGN_ROWS steps follow, each
// one LDS read, one compare, one add and one barrier with only LDS to wait for, the choices stay in registers and are stored
// after the burst's last step.  The first barrier of a burst waits for those stores and the burst's loads together: one memory
// latency per ALIGN_ROWS steps.  A row of the slab is N_max rounded up to 4 bytes, so that the four-column instantiation stores
// its four bytes at once.
// The backtrack is the last phase of the same launch.  The walk is a chain of dependent reads, so the workgroup first copies
// the part of the slab the next ALIGN_BT rows of the walk can reach (an ALIGN_BT x ALIGN_BT window that ends at the walk's
// current token) into LDS with all its lanes, and lane 0 walks there; it writes path and durations as it goes.
// One writer per element, fixed order, no atomics: two calls give the same bits and an utterance in a ragged batch gives the bits
// it gives alone.  Plain C++ and __syncthreads only, so the CPU suite runs this very source on the host stand-in (tests/hip_emu).
#include "common.h"

#define ALIGN_W 256                     /* lanes of the workgroup */
#define ALIGN_MAX_T 4096                /* frames at most */
#define ALIGN_MAX_C 4                   /* columns of a lane at most: ALIGN_W ALIGN_MAX_C = 1024 tokens */
#define ALIGN_ROWS 16                   /* rows of l loaded, and rows of choices stored, at a time */
#define ALIGN_BT 128                    /* rows of the walk per LDS window: 16 KiB */

template <int C>
__global__ void __launch_bounds__(ALIGN_W) align_kernel(const float* __restrict__ scores, long long sb, long long st,
                                                        const int* __restrict__ t_len, const int* __restrict__ n_len, int T_max,
                                                        int N_max, int* __restrict__ durations, float* __restrict__ score,
                                                        int* __restrict__ path, unsigned char* __restrict__ ws, int ldw,
                                                        unsigned long long* __restrict__ stamps) {
    __shared__ float edge[2][ALIGN_W];
    __shared__ unsigned char win[ALIGN_BT * ALIGN_BT];
    __shared__ int walk_n;
    const int b = blockIdx.x, l = threadIdx.x;
    const unsigned long long clk0 = wall_clock64();
    const int T = t2_clamp_count(t_len[b], T_max < ALIGN_MAX_T ? T_max : ALIGN_MAX_T);
    const int N = t2_clamp_count(n_len[b], N_max < C * ALIGN_W ? N_max : C * ALIGN_W);
    int* dur = durations + (long long)b * N_max;
    int* pth = path ? path + (long long)b * T_max : nullptr;
    for (int n = N + l; n < N_max; n += ALIGN_W) dur[n] = 0;
    if (pth)
        for (int t = T + l; t < T_max; t += ALIGN_W) pth[t] = -1;
    if (T < 1 || N < 1 || N > T) {                                          // uniform; the host refuses such lengths
        for (int n = l; n < N; n += ALIGN_W) dur[n] = 0;
        if (pth)
            for (int t = l; t < T; t += ALIGN_W) pth[t] = -1;
        if (l == 0) {
            score[b] = 0.0f;
            stamps[2 * b] = 0;
            stamps[2 * b + 1] = 0;
        }
        return;
    }
    const float* x = scores + b * sb;
    unsigned char* slab = ws + (long long)b * T_max * ldw;
    const float ninf = __uint_as_float(0xff800000u);
    const int n0 = l * C;

    // ---- the recurrence: row 0, then one barrier per row, ALIGN_ROWS rows at a time.  The loads are unconditional (rows beyond
    // T - 1 and columns beyond N - 1 read row T - 1 and column N - 1 again): what columns at and beyond N compute is never
    // looked at, and nothing to their left depends on them.
    float q[C];
    int oc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        oc[c] = n0 + c < N ? n0 + c : N - 1;
        q[c] = ninf;
    }
    if (l == 0) q[0] = x[0];
    edge[0][l] = q[C - 1];
    __syncthreads();
    for (int t0 = 1; t0 < T; t0 += ALIGN_ROWS) {
        float row[ALIGN_ROWS][C];
        unsigned bits[ALIGN_ROWS];
#pragma unroll
        for (int d = 0; d < ALIGN_ROWS; ++d)
#pragma unroll
            for (int c = 0; c < C; ++c) row[d][c] = x[(t0 + d < T ? t0 + d : T - 1) * st + oc[c]];
#pragma unroll
        for (int d = 0; d < ALIGN_ROWS; ++d) {
            const int t = t0 + d;
            if (t < T) {                                                    // uniform
                float adv = l > 0 ? edge[(t + 1) & 1][l - 1] : ninf;
                unsigned ch = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float stay = q[c];
                    float best = stay;                                      // the tie rule: staying wins
                    if (adv > best) {
                        best = adv;
                        ch |= 1u << (8 * c);
                    }
                    q[c] = row[d][c] + best;
                    adv = stay;
                }
                edge[t & 1][l] = q[C - 1];
                bits[d] = ch;
                __syncthreads();
            }
        }
        if (n0 < N) {
#pragma unroll
            for (int d = 0; d < ALIGN_ROWS; ++d)
                if (t0 + d < T) {
                    unsigned char* cell = slab + (long long)(t0 + d) * ldw + n0;
                    if (C == 1) *cell = (unsigned char)bits[d];
                    else *reinterpret_cast<unsigned*>(cell) = bits[d];      // columns n0 .. n0 + 3 < ldw, 4-byte aligned
                }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (n0 + c == N - 1) score[b] = q[c];
    __syncthreads();                                                        // the slab is this workgroup's own: visible to it now
    const unsigned long long clk1 = wall_clock64();

    // ---- the walk, ALIGN_BT rows at a time: rows t_hi .. t_hi - rows + 1 (>= 1), columns c0 .. n_hi of them in LDS
    int n_hi = N - 1, count = 0;
    for (int t_hi = T - 1; t_hi >= 1; t_hi -= ALIGN_BT) {
        const int rows = t_hi < ALIGN_BT ? t_hi : ALIGN_BT, c0 = n_hi - ALIGN_BT + 1;
        for (int e0 = l; e0 < rows * ALIGN_BT; e0 += ALIGN_W * ALIGN_ROWS) {   // ALIGN_ROWS loads in flight a lane, unconditional:
            unsigned char v[ALIGN_ROWS];                                        // an index past the window or left of column 0 is clamped
#pragma unroll
            for (int k = 0; k < ALIGN_ROWS; ++k) {
                int e = e0 + k * ALIGN_W;
                e = e < rows * ALIGN_BT ? e : rows * ALIGN_BT - 1;
                const int n = c0 + e % ALIGN_BT;
                v[k] = slab[(long long)(t_hi - e / ALIGN_BT) * ldw + (n < 0 ? 0 : n)];
            }
#pragma unroll
            for (int k = 0; k < ALIGN_ROWS; ++k)
                if (e0 + k * ALIGN_W < rows * ALIGN_BT) win[e0 + k * ALIGN_W] = v[k];
        }
        __syncthreads();
        if (l == 0) {
            int n = n_hi;
            for (int r = 0; r < rows; ++r) {
                const int t = t_hi - r;
                if (pth) pth[t] = n;
                ++count;
                bool advanced = (win[r * ALIGN_BT + n - c0] & 1) != 0;
                if (n == 0) advanced = false;                               // whatever the byte says, the walk stays inside
                else if (n == t) advanced = true;
                if (advanced) {
                    dur[n] = count;
                    count = 0;
                    --n;
                }
            }
            walk_n = n;
        }
        __syncthreads();
        n_hi = walk_n;
    }
    if (l == 0) {                                                           // row 0: n <= t all the way, so the token is 0
        if (pth) pth[0] = 0;
        dur[0] = count + 1;
        stamps[2 * b] = clk1 - clk0;
        stamps[2 * b + 1] = wall_clock64() - clk1;
    }
}

static long long align_slab_bytes(int B, int T_max, int N_max) { return t2_round_up((long long)B * T_max * t2_round_up(N_max, 4), 8); }

static int align_check(int B, int T_max, int N_max, char* msg) {
    const char* what = !(B >= 1 && B <= 1048576)        ? "1 to 2^20 utterances"
                       : !(T_max >= 1 && N_max >= 1)    ? "at least 1 frame and 1 token"
                       : !(T_max <= ALIGN_MAX_T)        ? "at most 4096 frames"
                       : !(N_max <= ALIGN_MAX_C * ALIGN_W) ? "at most 1024 tokens"
                                                        : nullptr;
    if (!what) return T2AMD_OK;
    snprintf(msg, 160, "monotonic_align: %s: B %d frames %d tokens %d", what, B, T_max, N_max);
    return T2AMD_ERR_ARG;
}

extern "C" int t2amd_align_limits(int* width, int* max_frames, int* max_tokens) {
    T2_REQUIRE(width && max_frames && max_tokens, "align_limits: null operand");
    *width = ALIGN_W;
    *max_frames = ALIGN_MAX_T;
    *max_tokens = ALIGN_MAX_C * ALIGN_W;
    return T2AMD_OK;
}

extern "C" int t2amd_align_workspace(int B, int T_max, int N_max, long long* bytes) {
    char msg[160];
    T2_REQUIRE(bytes, "align_workspace: null operand");
    if (align_check(B, T_max, N_max, msg) != T2AMD_OK) T2_FAIL(msg);
    *bytes = align_slab_bytes(B, T_max, N_max) + 16LL * B;                  // the choices, then two 64-bit clock counts an utterance
    return T2AMD_OK;
}

extern "C" int t2amd_monotonic_align_f32(const float* scores, long long sb, long long st, const int* t_len, const int* n_len, int B,
                                         int T_max, int N_max, int* durations, float* score, int* path, unsigned char* ws,
                                         long long ws_bytes, void* stream) {
    char msg[160];
    T2_REQUIRE(scores && t_len && n_len && durations && score && ws, "monotonic_align: null operand");
    if (align_check(B, T_max, N_max, msg) != T2AMD_OK) T2_FAIL(msg);
    T2_REQUIRE(t2_strides_cover(sb, st, B, T_max, N_max), "monotonic_align: score strides shorter than the matrix");
    const long long slab = align_slab_bytes(B, T_max, N_max);
    T2_REQUIRE(ws_bytes >= slab + 16LL * B, "monotonic_align: the workspace is smaller than t2amd_align_workspace asks for");
    T2_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "monotonic_align: the workspace is not aligned to 8 bytes");
    const long long sbytes = t2_span_bytes(sb, st, B, T_max, N_max);
    T2_REQUIRE(!t2_overlap(ws, ws_bytes, scores, sbytes) && !t2_overlap(durations, 4LL * B * N_max, scores, sbytes) &&
                   !t2_overlap(score, 4LL * B, scores, sbytes) && !(path && t2_overlap(path, 4LL * B * T_max, scores, sbytes)),
               "monotonic_align: outputs and workspace must not overlap the scores");
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(ws + slab);
    const int ldw = (int)t2_round_up(N_max, 4);
    if (N_max <= ALIGN_W)
        T2_LAUNCH(align_kernel<1>, dim3((unsigned)B), dim3(ALIGN_W), 0, (hipStream_t)stream, scores, sb, st, t_len, n_len, T_max,
                  N_max, durations, score, path, ws, ldw, stamps);
    else
        T2_LAUNCH(align_kernel<ALIGN_MAX_C>, dim3((unsigned)B), dim3(ALIGN_W), 0, (hipStream_t)stream, scores, sb, st, t_len, n_len,
                  T_max, N_max, durations, score, path, ws, ldw, stamps);
    T2_LAUNCH_CHECK();
    return T2AMD_OK;
}
