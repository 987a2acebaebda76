// A stand-alone program over csrc/predictor_rows.hip on the host stand-in, built with -fsanitize=address,undefined by
// tests/test_predictor_cpu.py: every kernel once on a ragged batch whose tensors are exactly as large as the entries say, at the
// widest geometry of tracks and taps and at the narrowest, so that a read or write beyond a row, a length or a workspace ends the
// program.  Exit status 0 = every entry returned 0.
#include <cstdio>
#include <vector>

#include "../../include/tacotron2_amd.h"

static int run(int B, int T, int C, int P, int k, const std::vector<int>& len) {
    std::vector<float> h(B * T * C), w(P * C, 0.5f), bias(P, 0.25f), y(B * T * P), g(B * T * P, 1.0f), dh(B * T * C), dw(P * C), db(P);
    for (size_t i = 0; i < h.size(); ++i) h[i] = 0.01f * (float)(i % 97);
    std::vector<float> v(B * T * P), image(P * k * C, 0.125f), cb(C, 0.5f), base(B * T * C, 1.0f), e(B * T * C), ge(B * T * C, 1.0f);
    std::vector<float> dbase(B * T * C), dv(B * T * P), dwe(C * P * k), dbe(C);
    for (size_t i = 0; i < v.size(); ++i) v[i] = 0.1f * (float)(i % 13);
    long long n = 0;
    int bad = 0;
    bad |= t2amd_pred_project_f32(h.data(), w.data(), bias.data(), len.data(), B, T, C, P, y.data(), nullptr);
    bad |= t2amd_pred_project_f32(h.data(), w.data(), nullptr, nullptr, B, T, C, P, y.data(), nullptr);
    bad |= t2amd_pred_project_bwd_f32(g.data(), w.data(), len.data(), B, T, C, P, dh.data(), nullptr);
    bad |= t2amd_predictor_workspace(B, T, C, P, 1, 1, &n);
    std::vector<unsigned char> ws((size_t)n);
    bad |= t2amd_pred_project_sums_f32(g.data(), h.data(), len.data(), B, T, C, P, dw.data(), db.data(), ws.data(), n, nullptr);
    bad |= t2amd_pred_embed_f32(v.data(), image.data(), cb.data(), base.data(), len.data(), B, T, C, P, k, e.data(), nullptr);
    bad |= t2amd_pred_embed_f32(v.data(), image.data(), nullptr, nullptr, nullptr, B, T, C, P, k, e.data(), nullptr);
    bad |= t2amd_pred_embed_bwd_f32(ge.data(), image.data(), len.data(), B, T, C, P, k, dbase.data(), dv.data(), nullptr);
    bad |= t2amd_pred_embed_bwd_f32(ge.data(), nullptr, len.data(), B, T, C, P, k, dbase.data(), nullptr, nullptr);
    bad |= t2amd_predictor_workspace(B, T, C, P, k, 2, &n);
    std::vector<unsigned char> wse((size_t)n);
    bad |= t2amd_pred_embed_sums_f32(ge.data(), v.data(), len.data(), B, T, C, P, k, dwe.data(), dbe.data(), wse.data(), n, nullptr);
    return bad;
}

int main() {
    int bad = run(3, 5, 36, 4, 9, {0, 2, 5});
    bad |= run(2, 70, 32, 1, 3, {70, 1});
    bad |= run(1, 3, 260, 3, 1, {3});
    if (bad) fprintf(stderr, "predictor_sanitize: an entry failed: %s\n", t2amd_last_error());
    return bad ? 1 : 0;
}
