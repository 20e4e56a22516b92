"""GPU: option "vits_slab_fuse" -- the vocoder front's LayerNorms (after an attention
out-projection and after FFN2) and its WaveNet gates sum the split-K slabs of the conv before
them, instead of that conv launching its own reduce.

Bar: bit equality.  Every case runs once with the option on and once off (the parent's
launches) and requires torch.equal on the audio and on the front's te, y, stats and z; the
counter "vits_slab_consumers" shows that the fused launches really ran (and none with the
option off).  The flow in_layer convs split 24 ways at these lengths, so the slab loops go
past one group of 8; the unsplit path (the consumer takes the plain form) is the large packed
batch of test_vits_gpu.py."""
import numpy as np
import pytest

from genie_tts_amd import synth
from tests.common import character

pytestmark = pytest.mark.gpu


def _engine(ver):
    from genie_tts_amd.engine import Engine
    w = character(ver)
    groups = {k: w[k] for k in ("t2s_encoder", "t2s", "vits") if k in w}
    if "prompt_encoder" in w:
        groups["prompt_encoder"] = w["prompt_encoder"]
    return Engine(groups, ver)


@pytest.fixture(scope="module")
def v2():
    e = _engine("v2")
    ge = e.ref_encode(synth.synth_ref_audio(32000 * 2 + 1234))   # once: the reference branch is not under test
    yield e, dict(ge=ge)
    e.set_vocoder_cus(0)
    e.close()


@pytest.fixture(scope="module")
def v2pp():
    e = _engine("v2ProPlus")
    yield e, dict(ge=synth.synth_ge(1024), ge_advanced=synth.synth_ge(512, "adv"))
    e.close()


def _utt(G, S, tag="sf"):
    txt = synth.synth_phones(S, f"{tag}{S}")
    sem = ((np.arange(G, dtype=np.int64) * 37 + 11) % 1024).reshape(1, 1, G)
    return txt, sem


def _single(e, fuse, G, S, speed, seed, kw):
    """One vocoder call: (audio, te, y, stats, z) and the fused launches it made."""
    txt, sem = _utt(G, S)
    frames = e.vits_frames(G, speed)
    e.set_option("vits_slab_fuse", fuse)
    try:
        n0 = e.counter("vits_slab_consumers")
        audio = e.vits_decode(txt, sem, noise_seed=seed, speed=speed, **kw).clone()
        bufs = [e.debug_copy(n, k).clone() for n, k in
                (("te", 192 * S), ("y", 192 * 2 * G), ("stats", 384 * frames), ("z", 192 * frames))]
        return [audio] + bufs, e.counter("vits_slab_consumers") - n0
    finally:
        e.set_option("vits_slab_fuse", 1)


def _same(e, G, S, speed, seed, kw, odd=False):
    import torch
    frames = e.vits_frames(G, speed)
    if odd:
        assert frames % 2 == 1 and (192 * frames) % 256 != 0
    on, n_on = _single(e, 1, G, S, speed, seed, kw)
    off, n_off = _single(e, 0, G, S, speed, seed, kw)
    # 2 x (3 + 3 + 6) encoder layers' LayerNorms and 4 x 4 gates, when every such conv splits
    assert n_on == 40 and n_off == 0, (n_on, n_off)
    assert on[0].shape == (640 * frames,)
    for name, a, b in zip(("audio", "te", "y", "stats", "z"), on, off):
        assert torch.equal(a, b), f"{name}: G {G} S {S} speed {speed} seed {seed}"
    assert torch.isfinite(on[0]).all() and float(on[0].abs().max()) > 0


@pytest.mark.parametrize("seed", [0x5EED, None])   # Philox noise, zero noise
@pytest.mark.parametrize("G,S,speed", [(8, 7, 1.0), (80, 45, 1.0), (8, 7, 1.25), (8, 7, 2.0)])
def test_v2_fused_equals_unfused(v2, G, S, speed, seed):
    """Odd S in the text branch; the bench's shape; T' = 13 and 9 after the resample (odd T at
    the gates, 192 T' no multiple of 256)."""
    e, kw = v2
    _same(e, G, S, speed, seed, kw, odd=speed != 1.0)


def test_v2proplus_fused_equals_unfused(v2pp):
    """The other conditioning widths."""
    e, kw = v2pp
    _same(e, 8, 7, 1.0, 0x5EED, kw)


def test_packed_batch_fused_equals_unfused(v2):
    """Three short items with the packed front (seg_front): gap columns and the per-segment vec."""
    import torch
    e, kw = v2
    items = []
    for i, (G, S) in enumerate([(8, 7), (13, 10), (9, 12)]):
        txt, sem = _utt(G, S, f"sfb{i}")
        items.append(dict(text_seq=txt, pred_semantic=sem, noise_seed=77 + i if i != 1 else None, **kw))
    outs = {}
    for fuse in (1, 0):
        e.set_option("vits_slab_fuse", fuse)
        try:
            p0, n0 = e.counter("vits_packed_fronts"), e.counter("vits_slab_consumers")
            outs[fuse] = [a.clone() for a in e.vits_decode_batch(items)]
            assert e.counter("vits_packed_fronts") == p0 + 1
            assert e.counter("vits_slab_consumers") - n0 == (40 if fuse else 0)
        finally:
            e.set_option("vits_slab_fuse", 1)
    for i, (a, b) in enumerate(zip(outs[1], outs[0])):
        assert torch.equal(a, b), f"item {i}"
        assert float(a.abs().max()) > 0


def test_async_vocoder_on_masked_stream_equals_sequential(v2):
    """The overlapped vocoder on the 64 vocoder CUs against the sequential call, option on."""
    import torch
    e, kw = v2
    txt, sem = _utt(80, 45)
    item = dict(text_seq=txt, pred_semantic=sem, noise_seed=0x5EED, **kw)
    e.set_vocoder_cus(0)
    seq = e.vits_decode(txt, sem, noise_seed=0x5EED, **kw).clone()
    e.set_vocoder_cus(64)
    try:
        n0 = e.counter("vits_slab_consumers")
        audio = e.vits_decode_async(item)
        e.vits_wait()
        assert e.counter("vits_slab_consumers") - n0 == 40
        assert torch.equal(audio, seq)
    finally:
        e.set_vocoder_cus(0)
