"""The cases the CPU and the GPU tests of the predictors and FastPitch share: builders with their float64 and
float32 restatements (tests/predictor_ref.py), runners that lay a ragged batch out with NaN beyond every utterance and call the
public functions on a device, the checks under the project's tolerance
max(4 x the float32 restatement's own largest error, 8 2^-24 max(1, largest |value| in float64)), and the small FastPitch of the
module tests with its torch restatement on one utterance alone."""
import math

import numpy as np
import torch

import fft_block_cases as fc
import predictor_ref as pr
from fft_block_cases import bits, layout  # noqa: F401

F32 = np.float32
PROJECT_C = (32, 36, 384, 4096)
PROJECT_P = (1, 2, 4)
PROJECT_T = (1, 3, 65)
EMBED_SHAPES = ((32, 1, 3), (384, 1, 3), (36, 2, 9), (64, 4, 1))
EMBED_T = (1, 2, 4, 5, 65)
RAGGED = (0, 1, 2, 5, 128, 130)


# ---- the thin projection -------------------------------------------------------------------------------------------------------
def project_batch(Ts, C, P, bias, seed=0):
    r = np.random.default_rng(seed * 7919 + sum(Ts) + 31 * len(Ts) + C + 5 * P)
    w = (r.standard_normal((P, C)) / np.sqrt(C)).astype(F32)
    b = r.standard_normal(P).astype(F32) if bias else None
    utts = []
    for T in Ts:
        h, g = r.standard_normal((T, C)).astype(F32), r.standard_normal((T, P)).astype(F32)
        u = dict(T=T, h=h, g=g)
        if T:
            dh, dw, db = pr.project_bwd64(h, w, g)
            u["f64"] = dict(y=pr.project64(h, w, b), dh=dh, dw=dw, db=db)
            u["f32"] = dict(y=pr.project32(h, w, b), dh=pr.project_dh32(g, w))
        utts.append(u)
    return dict(utts=utts, w=w, b=b, C=C, P=P)


def project_batch_sums(batch, T_max):
    live = [u for u in batch["utts"] if u["T"]]
    f64 = dict(dw=sum(u["f64"]["dw"] for u in live), db=sum(u["f64"]["db"] for u in live))
    dw, db = pr.project_sums32([u["g"] for u in batch["utts"]], [u["h"] for u in batch["utts"]], T_max)
    return f64, dict(dw=dw, db=db)


def _lengths(utts, dev, device_lengths):
    lens = [u["T"] for u in utts]
    return torch.tensor(lens, dtype=torch.int32, device=dev) if device_lengths else lens


def run_project(batch, dev, T=None, offset=0, device_lengths=True):
    """channel_project forward and backward on the batch -> dict of numpy y (B, T, P), dh (B, T, C), dw, db."""
    from tacotron2_amd import fastpitch
    utts = batch["utts"]
    T = T or max(1, max(u["T"] for u in utts))
    h = layout([u["h"] for u in utts], dev, T, offset).requires_grad_(True)
    g = layout([u["g"] for u in utts], dev, T, offset)
    w = torch.from_numpy(batch["w"]).to(dev).requires_grad_(True)
    b = None if batch["b"] is None else torch.from_numpy(batch["b"]).to(dev).requires_grad_(True)
    y = fastpitch.channel_project(h, w, b, _lengths(utts, dev, device_lengths))
    y.backward(g)
    out = dict(y=y.detach().cpu().numpy(), dh=h.grad.cpu().numpy(), dw=w.grad.cpu().numpy(), T=T)
    if b is not None:
        out["db"] = b.grad.cpu().numpy()
    return out


def _check(batch, out, per_row, sums, label, text, exact):
    """The per-row tensors per utterance with exact +0 in the padding, the sums for the batch; prints the FIGURE ratios."""
    worst = {}
    for bi, u in enumerate(batch["utts"]):
        T = u["T"]
        for n in per_row:
            if n not in out:
                continue
            assert not bits(out[n][bi, T:]).any(), (label, bi, n, "padding")
            if not T:
                continue
            if exact:
                assert np.array_equal(bits(out[n][bi, :T]), bits(u["f32"][n])), (label, bi, n)
            worst[n] = max(worst.get(n, 0.0), pr.error(out[n][bi, :T], u["f64"][n]) / pr.allowed(u["f32"][n], u["f64"][n]))
    f64, f32 = sums
    for n in ("dw", "db"):
        if n in out:
            if exact:
                assert np.array_equal(bits(out[n]), bits(f32[n])), (label, n)
            worst[n] = pr.error(out[n], f64[n]) / pr.allowed(f32[n], f64[n])
    print("FIGURE predictor %s%s: error / allowed %s" % (label, text, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    return worst


def check_project(batch, out, label="", exact=False):
    """Under the tolerance, and with ``exact`` bit for bit against the float32 restatement (the host stand-in)."""
    text = "project (C %d P %d bias %d, frames %s)" % (batch["C"], batch["P"], batch["b"] is not None,
                                                        ",".join(str(u["T"]) for u in batch["utts"][:8]))
    return _check(batch, out, ("y", "dh"), project_batch_sums(batch, out["T"]), label, text, exact)


# ---- the thin embedding --------------------------------------------------------------------------------------------------------
def embed_batch(Ts, C, P, k, bias, base, seed=0):
    r = np.random.default_rng(seed * 104729 + sum(Ts) + 17 * len(Ts) + C + 3 * P + k)
    w = (r.standard_normal((C, P, k)) / np.sqrt(P * k)).astype(F32)
    b = r.standard_normal(C).astype(F32) if bias else None
    utts = []
    for T in Ts:
        v, g = r.standard_normal((T, P)).astype(F32), r.standard_normal((T, C)).astype(F32)
        a = r.standard_normal((T, C)).astype(F32) if base else None
        u = dict(T=T, v=v, g=g, base=a)
        if T:
            dv, dw, db = pr.embed_bwd64(v, w, g)
            u["f64"] = dict(y=pr.embed64(v, w, b, a), dv=dv, dw=dw, db=db, dbase=g.astype(np.float64))
            u["f32"] = dict(y=pr.embed32(v, w, b, a), dv=pr.embed_dv32(g, w), dbase=g)
        utts.append(u)
    return dict(utts=utts, w=w, b=b, C=C, P=P, k=k, base=base)


def embed_batch_sums(batch, T_max):
    live = [u for u in batch["utts"] if u["T"]]
    f64 = dict(dw=sum(u["f64"]["dw"] for u in live), db=sum(u["f64"]["db"] for u in live))
    dw, db = pr.embed_sums32([u["g"] for u in batch["utts"]], [u["v"] for u in batch["utts"]], batch["w"].shape, T_max)
    return f64, dict(dw=dw, db=db)


def run_embed(batch, dev, T=None, offset=0, device_lengths=True):
    """scalar_embed forward and backward on the batch -> dict of numpy y, dbase (B, T, C), dv (B, T, P), dw, db."""
    from tacotron2_amd import fastpitch
    utts = batch["utts"]
    T = T or max(1, max(u["T"] for u in utts))
    v = layout([u["v"] for u in utts], dev, T, offset).requires_grad_(True)
    g = layout([u["g"] for u in utts], dev, T, offset)
    base = layout([u["base"] for u in utts], dev, T, offset).requires_grad_(True) if batch["base"] else None
    w = torch.from_numpy(batch["w"]).to(dev).requires_grad_(True)
    b = None if batch["b"] is None else torch.from_numpy(batch["b"]).to(dev).requires_grad_(True)
    y = fastpitch.scalar_embed(v, w, b, _lengths(utts, dev, device_lengths), base)
    y.backward(g)
    out = dict(y=y.detach().cpu().numpy(), dv=v.grad.cpu().numpy(), dw=w.grad.cpu().numpy(), T=T)
    if b is not None:
        out["db"] = b.grad.cpu().numpy()
    if base is not None:
        out["dbase"] = base.grad.cpu().numpy()
    return out


def check_embed(batch, out, label="", exact=False):
    text = "embed (C %d P %d k %d bias %d base %d, frames %s)" % (batch["C"], batch["P"], batch["k"], batch["b"] is not None, batch["base"],
                                                                  ",".join(str(u["T"]) for u in batch["utts"][:8]))
    return _check(batch, out, ("y", "dv", "dbase"), embed_batch_sums(batch, out["T"]), label, text, exact)


# ---- the modules in torch, one utterance alone ---------------------------------------------------------------------------------
SMALL = dict(n_symbols=11, n_mel=80, d_model=64, n_layer=2, n_head=1, d_head=32, d_inner=128, kernel_size=3, predictor_filter=64,
             predictor_kernel=3, predictor_layers=2, pitch_kernel=3)
TOKENS = (3, 7, 12)


def predictor_ref(sd, prefix, x, n_layers=2):
    """TemporalPredictor on one utterance (T, C) from the state dict, in x's dtype -> (T, n_predictions)."""
    F = torch.nn.functional
    p = lambda n: sd[prefix + n].to(x.dtype)                                # noqa: E731
    h = x
    for i in range(n_layers):
        w = p("layers.%d.conv.weight" % i)
        h = F.relu(F.conv1d(h.t()[None], w, p("layers.%d.conv.bias" % i), padding=w.shape[2] // 2))[0].t()
        h = F.layer_norm(h, (h.shape[1],), p("layers.%d.norm.weight" % i), p("layers.%d.norm.bias" % i), 1e-5)
    return F.linear(h, p("fc.weight"), p("fc.bias"))


def transformer_ref(sd, prefix, h, cfg):
    h = h + fc.pos_emb_ref(h.shape[0], cfg["d_model"], h.dtype)
    for i in range(cfg["n_layer"]):
        h = fc.block_ref(sd, "%slayers.%d." % (prefix, i), h, cfg["n_head"], cfg["d_head"], (cfg["kernel_size"],) * 2, False)
    return h


def embed_ref(sd, prefix, v, base):
    """The pitch embedding of one utterance: v (N,), base (N, d)."""
    F = torch.nn.functional
    w = sd[prefix + "weight"].to(base.dtype)
    return base + F.conv1d(v.to(base.dtype)[None, None], w, sd[prefix + "bias"].to(base.dtype), padding=w.shape[2] // 2)[0].t()


def encode_ref(sd, cfg, ids):
    """-> enc (N, d), log_dur (N,), pitch_pred (N,) of one utterance."""
    enc = transformer_ref(sd, "encoder.", sd["encoder.word_emb.weight"][ids], cfg)
    return enc, predictor_ref(sd, "duration_predictor.", enc)[:, 0], predictor_ref(sd, "pitch_predictor.", enc)[:, 0]


def decode_ref(sd, cfg, enc, durations, pitch):
    """-> mel (sum of durations, n_mel) of one utterance."""
    h = embed_ref(sd, "pitch_emb.", pitch, enc)
    frames = torch.repeat_interleave(h, torch.as_tensor(durations, dtype=torch.long), dim=0)
    dec = transformer_ref(sd, "decoder.", frames, cfg)
    return torch.nn.functional.linear(dec, sd["proj.weight"].to(dec.dtype), sd["proj.bias"].to(dec.dtype))


def small_model(seed=11, dur_bias=None):
    """The small FastPitch of the module tests on the host, every parameter moved off its initial value, and its state dict."""
    from tacotron2_amd import fastpitch
    torch.manual_seed(seed)
    model = fastpitch.FastPitch(**SMALL)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
        model.encoder.word_emb.weight[0].zero_()
        if dur_bias is not None:
            model.duration_predictor.fc.bias.fill_(dur_bias)
    return model, {k: v.detach().clone() for k, v in model.state_dict().items()}


def small_batch(seed=7):
    """Tokens (3, 7, 12): symbols 1 .. 10, durations 0 .. 4 with a zero-duration token in every utterance, token-rate pitch and the
    gradients of mel (per utterance), log-duration and pitch predictions."""
    r = np.random.default_rng(seed)
    utts = []
    for n in TOKENS:
        d = r.integers(0, 5, (n,))
        d[0], d[n - 1] = 2, 0
        T = int(d.sum())
        utts.append(dict(N=n, ids=r.integers(1, 11, (n,)), durations=d, T=T, pitch=r.standard_normal(n).astype(F32),
                         g_mel=r.standard_normal((T, SMALL["n_mel"])).astype(F32), g_dur=r.standard_normal(n).astype(F32),
                         g_pitch=r.standard_normal(n).astype(F32), mel=r.standard_normal((T, SMALL["n_mel"])).astype(F32)))
    return utts


def pad_tokens(utts, key, dev, dtype, fill=0):
    N = max(u["N"] for u in utts)
    out = torch.full((len(utts), N), fill, dtype=dtype)
    for b, u in enumerate(utts):
        out[b, :u["N"]] = torch.from_numpy(np.asarray(u[key])).to(dtype)
    return out.to(dev)


def infer_reference(sd, utts, pace, max_duration=75, margin=1e-3):
    """The float64 free-running durations of every utterance, with the assertion that no token's (exp(log_dur) - 1) / pace lies
    within ``margin`` of a half-integer, so that float32 rounds to the same integers.  -> list of int arrays."""
    out = []
    for u in utts:
        leaves = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
        _, log_dur, _ = encode_ref(leaves, SMALL, torch.from_numpy(u["ids"]))
        d = (torch.exp(log_dur) - 1.0) / pace
        frac = (d - torch.floor(d) - 0.5).abs()
        assert float(frac.min()) > margin, (u["N"], pace, float(frac.min()))
        out.append(torch.round(d).clamp(0, max_duration).to(torch.int64).numpy())
    return out


def loss_ref(mel_out, mel, log_dur, durations, pitch_pred, pitch, scales=(0.1, 0.1), energy=None):
    """FastPitchLoss as a float64 loop over lists of per-utterance arrays -> (total, parts)."""
    se = dict(mel=0.0, duration=0.0, pitch=0.0, energy=0.0)
    frames = tokens = 0
    for b in range(len(mel_out)):
        for t in range(len(mel_out[b])):
            frames += 1
            for c in range(mel_out[b].shape[1]):
                se["mel"] += (float(mel_out[b][t, c]) - float(mel[b][t, c])) ** 2
        for n in range(len(log_dur[b])):
            tokens += 1
            se["duration"] += (float(log_dur[b][n]) - math.log(1.0 + float(durations[b][n]))) ** 2
            se["pitch"] += (float(pitch_pred[b][n]) - float(pitch[b][n])) ** 2
            if energy is not None:
                se["energy"] += (float(energy[0][b][n]) - float(energy[1][b][n])) ** 2
    parts = dict(mel=se["mel"] / (max(frames, 1) * mel_out[0].shape[1]), duration=se["duration"] / max(tokens, 1),
                 pitch=se["pitch"] / max(tokens, 1))
    total = parts["mel"] + scales[0] * parts["duration"] + scales[1] * parts["pitch"]
    if energy is not None:
        parts["energy"] = se["energy"] / max(tokens, 1)
        total += energy[2] * parts["energy"]
    return total, parts
