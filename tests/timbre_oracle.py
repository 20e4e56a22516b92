"""The CPU oracle of timbre fusion (tests/test_timbre_mix_gpu.py): the numpy float32 chain of
gsv_ge_mix, the fused embedding from oracle/restate.py's per-clip encoders combined in float64,
and the vocoder driven with a given embedding, assembled from VitsModel's own methods."""
import numpy as np
import torch

from oracle import restate as R


def mix_chain_np(xs, w):
    """include/genie_engine.h, gsv_ge_mix: acc = w_0 * x_0; acc = acc + w_i * x_i, every multiply
    and add a float32 operation of its own."""
    w = np.asarray(w, np.float32)
    acc = w[0] * np.asarray(xs[0], np.float32)
    for wi, x in zip(w[1:], xs[1:]):
        p = wi * np.asarray(x, np.float32)
        acc = acc + p
    assert acc.dtype == np.float32
    return acc


def clip_ge(w, vm, ver, clip, sv=None):
    """One clip's global embedding by the oracle, float32 [D]."""
    if ver == "v2":
        return R.ref_encoder(R.spectrogram(torch.from_numpy(np.asarray(clip, np.float32))), vm.w,
                             "vq_model.ref_enc.").numpy().reshape(-1)
    return R.prompt_encoder(w["prompt_encoder"], clip, sv)[0].numpy().reshape(-1)


def project(w, ge):
    """ge_to512 of a ge [1024] with the oracle's weights, in float64 -> float32 [512]."""
    W = np.asarray(w["prompt_encoder"]["ge_to512.weight"], np.float64)
    b = np.asarray(w["prompt_encoder"]["ge_to512.bias"], np.float64)
    return (W @ np.asarray(ge, np.float64) + b).astype(np.float32)


def fused(w, ver, ges, weights):
    """(ge, ge_advanced or None): the clips' oracle embeddings combined in float64 with the
    float32 weights the device multiplies; on V2ProPlus ge_advanced is the projection of the mix."""
    acc = sum(np.float64(wi) * np.asarray(g, np.float64) for wi, g in zip(np.asarray(weights, np.float32), ges))
    ge = acc.astype(np.float32)
    return ge, (None if ver == "v2" else project(w, acc))


def wave(vm, ver, text_seq, sem, ge, ge_adv=None):
    """The vocoder with zero noise on a given embedding: text_encoder -> flow_reverse -> generator
    (VitsModel.__call__ behind its reference branch; z_p = m_p at eps = 0)."""
    ge_t = torch.from_numpy(np.asarray(ge, np.float32).reshape(1, -1, 1))
    ge_m = ge_t if ver == "v2" else torch.from_numpy(np.asarray(ge_adv, np.float32).reshape(1, -1, 1))
    m_p, _ = vm.text_encoder(sem, text_seq, ge_m)
    return vm.generator(vm.flow_reverse(m_p, ge_t), ge_t)[0, 0].numpy()
