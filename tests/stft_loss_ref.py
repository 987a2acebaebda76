"""The multi-resolution STFT loss (tacotron2_amd.audio.MultiResolutionSTFTLoss) restated in torch under
autograd, in the dtype of its input (float64 is the reference, float32 the yardstick of the fp32 limit).  Window and basis are the
project's (``audio.fourier_basis``).  Per resolution r = (L, hop, win), with the sums over the frames j < n_{r,b} and all bins:

    m = sqrt(max(re^2 + im^2, eps));  A = sum (m_y - m_x)^2;  Bn = sum m_y^2;  sc = sqrt(A) / sqrt(Bn);  lm = sum |ln m_x - ln m_y| / C
    loss = (1/R) sum_r (sc_weight sc_r + mag_weight lm_r)

Three subgradients are definitions, stated here exactly as on the device: the clamp passes the gradient where p >= eps (torch's
own rule for clamp(min=)) and gives 0 below; sign(0) = 0 (torch's own rule for abs); where A == 0 the spectral-convergence term is
the constant 0 (torch's sqrt gives NaN there).  Bn == 0 is refused.
"""
import functools

import torch

from tacotron2_amd import audio

RESOLUTIONS = ((64, 16, 48), (128, 40, 100), (32, 10, 24))     # 2F = 130 and 34 are no multiples of 4; hop 10 neither
CASES = {                                                       # name -> (B, T, sample lengths)
    'A': (1, 65, None),                                         # one more than max L / 2: both mirrors fold onto the same samples
    'B': (1, 2125, None),
    'C': (3, 1500, None),
    'Cr': (3, 1500, (1500, 333, 800)),
}
X_SEED, Y_SEED = 7, 11
PARITY_EPS = 1e-12                                              # the smallest power over the cases is about 3e-8
MARGIN = 30.0                                                   # |ln m_x - ln m_y| over its own float32-vs-float64 difference


def signals(name):
    """(x, y) float64 (B, T): x = clamp(0.1 randn), y = 0.7 x + 0.7 clamp(0.1 randn), a target correlated with the input."""
    B, T, _ = CASES[name]
    x = torch.clamp(0.1 * torch.randn(B, T, generator=torch.Generator().manual_seed(X_SEED), dtype=torch.float64), -1.0, 1.0)
    e = torch.clamp(0.1 * torch.randn(B, T, generator=torch.Generator().manual_seed(Y_SEED), dtype=torch.float64), -1.0, 1.0)
    return x, 0.7 * x + 0.7 * e


@functools.lru_cache(maxsize=None)
def basis_of(L, win, dtype, device):
    """The project's (2F, L) table in a dtype on a device, built once: a caller that times the restatement times no host work."""
    return torch.from_numpy(audio.fourier_basis(L, win)).to(dtype=dtype, device=device)


def spectrum(sig, res):
    """(B, T) -> (B, n, 2F) rows [re | im] of ``audio.STFT(*res)``'s transform, in sig's dtype."""
    L, hop, win = (int(v) for v in res)
    basis = basis_of(L, win, sig.dtype, sig.device)
    B, T = sig.shape
    x = torch.nn.functional.pad(sig.view(B, 1, 1, T), (L // 2, L // 2, 0, 0), mode='reflect').view(B, -1)
    return x.unfold(-1, L, hop) @ basis.t()


def frame_counts(B, T, res, lens):
    n = T // res[1] + 1
    return [n if lens is None else min(n, int(v) // res[1] + 1) for v in (lens or [T] * B)]


def frame_mask(B, T, res, lens, device=None):
    n = T // res[1] + 1
    cnt = torch.tensor(frame_counts(B, T, res, lens), device=device)
    return torch.arange(n, device=device)[None, :] < cnt[:, None]


def power_mag(spec, eps):
    F = spec.shape[-1] // 2
    p = spec[..., :F] ** 2 + spec[..., F:] ** 2
    return p, torch.sqrt(torch.clamp(p, min=eps))


def sums(spec_x, spec_y, mask, eps):
    """A, Bn, sum |ln m_x - ln m_y| over the frames inside ``mask`` (B, n)."""
    _, mx = power_mag(spec_x, eps)
    _, my = power_mag(spec_y, eps)
    w = mask[..., None].to(mx.dtype)
    return (((my - mx) ** 2) * w).sum(), ((my ** 2) * w).sum(), ((torch.log(mx) - torch.log(my)).abs() * w).sum()


def loss_from_spectra(specs_x, specs_y, masks, sc_weight=1.0, mag_weight=1.0, eps=1e-7):
    """-> (loss, (R, 2) terms) from the spectra (B, n_r, 2 F_r) of every resolution."""
    total, terms = 0.0, []
    for sx, sy, mask in zip(specs_x, specs_y, masks):
        A, Bn, Lm = sums(sx, sy.detach(), mask, eps)
        if Bn.item() == 0.0:
            raise ValueError("an all-silent target: sum m_y^2 == 0")
        sc = A.detach() * 0.0 if A.item() == 0.0 else torch.sqrt(A) / torch.sqrt(Bn)
        lm = Lm / (int(mask.sum().item()) * (sx.shape[-1] // 2))
        total = total + sc_weight * sc + mag_weight * lm
        terms.append(torch.stack([sc.detach(), lm.detach()]))
    return total / len(specs_x), torch.stack(terms)


def loss(x, y, resolutions=RESOLUTIONS, lens=None, sc_weight=1.0, mag_weight=1.0, eps=1e-7):
    """-> (loss, (R, 2) terms); x (B, T) carries the gradient, y (B, >= T) does not."""
    B, T = x.shape
    y = y[:, :T].detach().to(x.dtype)
    return loss_from_spectra([spectrum(x, r) for r in resolutions], [spectrum(y, r) for r in resolutions],
                             [frame_mask(B, T, r, lens, x.device) for r in resolutions], sc_weight, mag_weight, eps)


def loss_and_grad(x, y, resolutions=RESOLUTIONS, lens=None, sc_weight=1.0, mag_weight=1.0, eps=1e-7):
    x = x.detach().clone().requires_grad_(True)
    val, terms = loss(x, y, resolutions, lens, sc_weight, mag_weight, eps)
    val.backward()
    return val.detach(), terms, x.grad


def spec_rows(sig, res):
    """float32 (B n, 2F) rows, the layout the kernels read."""
    s = spectrum(sig, res)
    return s.reshape(-1, s.shape[-1]).float().contiguous()
