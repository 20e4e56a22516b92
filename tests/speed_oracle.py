"""The speech-rate resample restated in numpy, and the VITS oracle with it inserted.

`interp_linear_np` is the formula of include/genie_engine.h (ATen's align_corners=False
coordinates in float32) with every operation rounded to float32 on its own -- what the
engine's k_interp_linear computes, bit for bit.  tests/test_speed_host.py pins it to
torch.nn.functional.interpolate within a derived bound; the GPU tests compare against it.
"""
from __future__ import annotations

import numpy as np


def interp_linear_np(y: np.ndarray, t_out: int) -> np.ndarray:
    """y f32 [..., T] -> [..., t_out]."""
    y = np.asarray(y, np.float32)
    T = y.shape[-1]
    f = np.float32
    scale = f(T) / f(t_out)
    j = np.arange(t_out, dtype=np.float32)
    src = np.maximum(scale * (j + f(0.5)) - f(0.5), f(0.0))
    i0 = np.minimum(src.astype(np.int32), T - 1)
    i1 = i0 + (i0 < T - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f(1.0) - l1
    assert src.dtype == l0.dtype == np.float32
    return l0 * y[..., i0] + l1 * y[..., i1]


def interp_bound(y: np.ndarray, t_out: int) -> np.ndarray:
    """Per-element bound on |interp_linear_np - F.interpolate| (ATen rounds the source
    coordinate differently: it multiplies by a precomputed scale in another order).  The
    coordinate differs by at most 4 ulp of T (4 * 2^-23 * T), which moves the result by that
    times the larger adjacent slope s = max(|y[i0+1] - y[i0]|, |y[i0] - y[i0-1]|); the two
    products and the sum add 2^-22 * max(|y[i0]|, |y[i1]|)."""
    y = np.asarray(y, np.float64)
    T = y.shape[-1]
    scale = np.float32(T) / np.float32(t_out)
    j = np.arange(t_out, dtype=np.float32)
    src = np.maximum(scale * (j + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    i0 = np.minimum(src.astype(np.int32), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    im = np.maximum(i0 - 1, 0)
    s = np.maximum(np.abs(y[..., i1] - y[..., i0]), np.abs(y[..., i0] - y[..., im]))
    return 4 * 2.0 ** -23 * T * s + 2.0 ** -22 * np.maximum(np.abs(y[..., i0]), np.abs(y[..., i1]))


def vits_oracle(vm, text_seq, pred_semantic, frames=None, ref_audio=None, ge=None, ge_advanced=None, eps=None,
                noise_scale: float = 0.5):
    """oracle.restate.VitsModel.__call__ with VitsModel.text_encoder's body restated and the
    numpy resample to `frames` inserted between encoder2 and proj (frames None: no resample;
    then it must equal VitsModel.__call__ exactly -- the tests assert that first)."""
    import torch
    from oracle import restate as R
    w = vm.w
    if vm.version == "v2":
        spec = R.spectrogram(torch.from_numpy(np.asarray(ref_audio, np.float32)))
        ge_t = R.ref_encoder(spec, w, "vq_model.ref_enc.")
        ge_m = ge_t
    else:
        ge_t = torch.from_numpy(np.asarray(ge, np.float32))
        ge_m = torch.from_numpy(np.asarray(ge_advanced, np.float32))
    # ---- VitsModel.text_encoder
    p = "vq_model.enc_p."
    codes = torch.from_numpy(np.asarray(pred_semantic, np.int64)).reshape(-1)
    q = w["vq_model.quantizer.vq.layers.0._codebook.embed"][codes].t().unsqueeze(0)
    q = torch.repeat_interleave(q, 2, dim=2)
    y = R._conv(q, w[p + "ssl_proj.weight"], w[p + "ssl_proj.bias"])
    y = R._attn_encoder(y, w, p + "encoder_ssl", vm.cfg.n_ssl_layers)
    t = torch.from_numpy(np.asarray(text_seq, np.int64)).reshape(-1)
    te = w[p + "text_embedding.weight"][t].t().unsqueeze(0)
    te = R._attn_encoder(te, w, p + "encoder_text", vm.cfg.n_text_layers)
    m = p + "mrte."
    ssl_enc = R._conv(y, w[m + "c_pre.weight"], w[m + "c_pre.bias"])
    text_enc = R._conv(te, w[m + "text_pre.weight"], w[m + "text_pre.bias"])
    x = R._mha_plain(ssl_enc, text_enc, w, m + "cross_attention.", 4) + ssl_enc + ge_m
    y = R._conv(x, w[m + "c_post.weight"], w[m + "c_post.bias"])
    y = R._attn_encoder(y, w, p + "encoder2", vm.cfg.n_enc2_layers)
    if frames is not None and frames != y.shape[-1]:
        y = torch.from_numpy(interp_linear_np(y.numpy(), frames))
    stats = R._conv(y, w[p + "proj.weight"], w[p + "proj.bias"])
    m_p, logs_p = stats[:, :192], stats[:, 192:]
    # ---- the rest of VitsModel.__call__
    e = torch.zeros_like(m_p) if eps is None else torch.from_numpy(np.asarray(eps, np.float32))
    z_p = m_p + (e * torch.exp(logs_p)) * noise_scale
    z = vm.flow_reverse(z_p, ge_t)
    return vm.generator(z, ge_t)[0, 0]
