// A stand-alone program over csrc/fft_block_rows.hip on the host stand-in, built with -fsanitize=address,undefined by
// tests/test_fft_block_cpu.py: every rows kernel once on a ragged batch whose tensors are exactly as large as the entries say,
// so that a read or write beyond a row, a length or a workspace ends the program.  Exit status 0 = every entry returned 0.
#include <cstdio>
#include <vector>

#include "../../include/tacotron2_amd.h"

int main() {
    const int B = 3, T = 5, C = 36, Cin = 32, Cout = 64, k = 3;
    const std::vector<int> len = {0, 2, 5};
    std::vector<float> x(B * T * C, 0.5f), res(B * T * C, 0.25f), w(C, 1.0f), b(C, 0.0f), y(B * T * C), z(B * T * C), g(B * T * C, 1.0f);
    std::vector<float> dz(B * T * C), mean(B * T), rstd(B * T), db(C), dw(C);
    for (int i = 0; i < B * T * C; ++i) x[i] = 0.01f * (float)(i % 97);
    long long n = 0;
    int bad = 0;
    bad |= t2amd_ffb_add_ln_f32(x.data(), res.data(), w.data(), b.data(), len.data(), B, T, C, 1e-5f, y.data(), z.data(), mean.data(),
                                rstd.data(), nullptr);
    bad |= t2amd_ffb_add_ln_f32(x.data(), nullptr, nullptr, nullptr, len.data(), B, T, C, 1e-5f, y.data(), nullptr, nullptr, nullptr, nullptr);
    bad |= t2amd_ffb_add_ln_bwd_f32(g.data(), z.data(), mean.data(), rstd.data(), w.data(), len.data(), B, T, C, dz.data(), nullptr);
    bad |= t2amd_fft_block_workspace(B, T, C, C, 1, 2, &n);
    std::vector<unsigned char> ws((size_t)n);
    bad |= t2amd_ffb_colsum_f32(g.data(), z.data(), mean.data(), rstd.data(), len.data(), B, T, C, db.data(), dw.data(), ws.data(), n, nullptr);
    bad |= t2amd_ffb_colsum_f32(g.data(), nullptr, nullptr, nullptr, len.data(), B, T, C, db.data(), nullptr, ws.data(), n, nullptr);
    bad |= t2amd_ffb_relu_mask_f32(g.data(), x.data(), len.data(), B, T, C, dz.data(), nullptr);
    bad |= t2amd_fft_block_workspace(B, T, Cin, Cout, k, 1, &n);
    std::vector<unsigned char> slab((size_t)n);
    std::vector<float> gc(B * T * Cout, 1.0f), dwc(Cout * Cin * k);
    const long long part = n - 4LL * k * Cin * Cout;                         // one slice at this size: [slab | partials]
    bad |= t2amd_ffb_transpose_f32(gc.data(), len.data(), B, T, Cout, reinterpret_cast<float*>(slab.data()), part, nullptr);
    bad |= t2amd_ffb_dw_finish_f32(reinterpret_cast<const float*>(slab.data() + part), 1, Cin, Cout, k, dwc.data(), nullptr);
    if (bad) fprintf(stderr, "fft_block_sanitize: an entry failed: %s\n", t2amd_last_error());
    return bad ? 1 : 0;
}
