"""GPU: the speech-rate control (`speed`) -- the resample kernel alone, the waveform at
odd and otherwise unaligned frame counts against the oracle, and every vocoder path.

The oracle is oracle/restate.py's VitsModel with the numpy restatement of the resample
(tests/speed_oracle.py, pinned to F.interpolate by tests/test_speed_host.py) inserted
between encoder2 and proj; test_oracle_restatement_is_anchored asserts that without a
resample it is VitsModel.__call__ exactly.  T' always comes from Engine.vits_frames
(gsv_vits_frames, the one place it is computed).
"""
import ctypes

import numpy as np
import pytest

from genie_tts_amd import synth
from tests.common import character
from tests.speed_oracle import interp_linear_np, vits_oracle

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4


def _close(got, want, what=""):
    """test_vits_gpu.py's rule for a segmented-batch result vs the utterance decoded alone."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    rel = float(np.sqrt(np.mean((got - want) ** 2)) / max(1e-12, np.sqrt(np.mean(want ** 2))))
    assert rel <= 1e-5 and np.abs(got - want).max() <= 1e-4, f"{what}: rel rms {rel:.2e}"


@pytest.fixture(scope="module", params=["v2", "v2ProPlus"])
def setup(request):
    from genie_tts_amd.engine import Engine
    from oracle import restate as R
    ver = request.param
    w = character(ver)
    groups = {k: w[k] for k in ("t2s_encoder", "t2s", "vits") if k in w}
    if "prompt_encoder" in w:
        groups["prompt_encoder"] = w["prompt_encoder"]
    e = Engine(groups, ver)
    vm = R.VitsModel(w["vits"], ver)
    yield ver, e, vm, w
    e.close()


def _cond(ver):
    if ver == "v2":
        return dict(ref_audio=synth.synth_ref_audio(32000 * 2 + 1234))
    return dict(ge=synth.synth_ge(1024), ge_advanced=synth.synth_ge(512, "adv"))


def _utt(G, S, tag="sp"):
    txt = synth.synth_phones(S, f"{tag}{S}")
    sem = ((np.arange(G, dtype=np.int64) * 37 + 11) % 1024).reshape(1, 1, G)
    return txt, sem


def _check_wave(out, ref, frames, what=""):
    assert out.shape == (640 * frames,) == ref.shape, what
    rms = float(np.sqrt(np.mean((out - ref) ** 2)))
    print(f"{what}: T' {frames}, rms {rms:.3e}, max {np.abs(out - ref).max():.3e}")
    assert rms <= RMS_TOL, f"{what}: rms {rms:.3e} (signal rms {np.sqrt(np.mean(ref ** 2)):.3e})"
    assert np.abs(out - ref).max() < 2e-3, what


def test_oracle_restatement_is_anchored(setup):
    ver, _, vm, _ = setup
    txt, sem = _utt(8, 10)
    eps = synth.rng_for("anchor").standard_normal((1, 192, 16)).astype(np.float32)
    kw = _cond(ver)
    assert np.array_equal(vits_oracle(vm, txt, sem, eps=eps, **kw).numpy(), vm(txt, sem, eps=eps, **kw).numpy())
    assert np.array_equal(vits_oracle(vm, txt, sem, frames=16, **kw).numpy(), vm(txt, sem, **kw).numpy())


@pytest.mark.parametrize("T", [2, 3, 16, 17, 160])
def test_interp_kernel_alone_bit_equal(setup, T):
    """gsv_debug_interp_linear on [192][T] against the numpy restatement, bit for bit; the
    T' of speeds 0.5 / 0.8 / 1.25 / 2.0, and T' = T (the identity)."""
    import torch
    from genie_tts_amd.engine import _check, lib
    _, e, _, _ = setup
    y = np.random.default_rng(100 + T).standard_normal((192, T)).astype(np.float32)
    x = torch.from_numpy(y).to(e.dev)
    for sp in (0.5, 0.8, 1.25, 2.0, 1.0):
        To = int(T / float(np.float32(sp))) + 1 if sp != 1.0 else T    # odd T too: not only 2 n_sem
        if T % 2 == 0:
            assert To == e.vits_frames(T // 2, sp)
        out = torch.full((192, To), float("nan"), dtype=torch.float32, device=e.dev)
        _check(lib().gsv_debug_interp_linear(ctypes.c_void_p(x.data_ptr()), 192, T, To,
                                             ctypes.c_void_p(out.data_ptr()),
                                             ctypes.c_void_p(torch.cuda.current_stream(e.dev).cuda_stream)),
               "gsv_debug_interp_linear")
        torch.cuda.synchronize(e.dev)
        assert np.array_equal(out.cpu().numpy(), interp_linear_np(y, To)), (T, sp, To)


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("G,S,speed", [(8, 10, 0.5), (8, 10, 0.8), (8, 10, 1.25), (8, 10, 2.0), (80, 45, 0.9),
                                       (80, 45, 1.1)])
def test_vits_waveform_at_speed(setup, G, S, speed, noise):
    ver, e, vm, _ = setup
    txt, sem = _utt(G, S)
    frames = e.vits_frames(G, speed)
    eps = synth.rng_for(f"speps{G}{speed}").standard_normal((1, 192, frames)).astype(np.float32) if noise else None
    kw = _cond(ver)
    ref = vits_oracle(vm, txt, sem, frames=frames, eps=eps, **kw).numpy()
    out = e.vits_decode(txt, sem, eps=eps, speed=speed, **kw).cpu().numpy()
    _check_wave(out, ref, frames, f"G {G} speed {speed} noise {noise}")


@pytest.mark.parametrize("convh,fused", [(0, 0), (1, 0), (1, 1)])
def test_vits_waveform_conv_paths_at_odd_frames(setup, convh, fused):
    """The conv-path settings test_vits_waveform_conv_paths cycles, at an odd T' (G = 40 at
    speed 1.25: T' = 65): the f32 MFMA path, the split-fp16 path, the fused MRF pairs."""
    ver, e, vm, _ = setup
    G, S, speed = 40, 30, 1.25
    txt, sem = _utt(G, S, "spc")
    frames = e.vits_frames(G, speed)
    assert frames % 2 == 1
    eps = synth.rng_for("spc-eps").standard_normal((1, 192, frames)).astype(np.float32)
    kw = _cond(ver)
    ref = vits_oracle(vm, txt, sem, frames=frames, eps=eps, **kw).numpy()
    e.set_option("convh", convh)
    e.set_option("mrf_fused", fused)
    try:
        out = e.vits_decode(txt, sem, eps=eps, speed=speed, **kw).cpu().numpy()
    finally:
        e.set_option("convh", 1)
        e.set_option("mrf_fused", 1)
    _check_wave(out, ref, frames, f"convh {convh} fused {fused}")


def test_speed_one_is_untouched(setup):
    """gsv_vits_decode_item with speed 0 and 1.0 (through _vits_item) against gsv_vits_decode."""
    from genie_tts_amd.engine import _check, _stream, lib
    ver, e, _, _ = setup
    txt, sem = _utt(24, 16, "sp1")
    eps = synth.rng_for("sp1-eps").standard_normal((1, 192, 48)).astype(np.float32)
    kw = _cond(ver)
    for ep in (None, eps):
        want = e.vits_decode(txt, sem, eps=ep, **kw).cpu().numpy()
        for sp in (0.0, 1.0):
            item, keep, audio = e._vits_item(dict(text_seq=txt, pred_semantic=sem, eps=ep, speed=sp, **kw))
            assert item.speed == sp and audio.shape == (1280 * 24,)
            _check(lib().gsv_vits_decode_item(e.h, ctypes.byref(item), ctypes.c_float(0.5), _stream()),
                   "gsv_vits_decode_item")
            assert np.array_equal(audio.cpu().numpy(), want), sp


def test_every_path_agrees(setup):
    """Three utterances at speeds 0.8 / 1.0 / 1.25 (eps, no noise, Philox): the lanes
    (seg_vocoder 0) and the overlapped calls give the single calls bit for bit; the
    segmented generator pass matches under _close, with seg_front 0 and 1 (a batch with a
    resampled item declines to pack, so both run the fronts per item)."""
    ver, e, _, _ = setup
    kw0 = _cond(ver)
    kw = dict(ge=e.ref_encode(kw0["ref_audio"])) if ver == "v2" else kw0   # packable conditioning
    items = []
    for i, (G, S, sp) in enumerate([(20, 12, 0.8), (33, 25, 1.0), (9, 8, 1.25)]):
        txt, sem = _utt(G, S, f"spa{i}")
        it = dict(text_seq=txt, pred_semantic=sem, speed=sp, **kw)
        if i == 0:
            it["eps"] = synth.rng_for("spa-eps").standard_normal((1, 192, e.vits_frames(G, sp))).astype(np.float32)
        elif i == 2:
            it["noise_seed"] = 4242
        items.append(it)
    singles = [e.vits_decode(it["text_seq"], it["pred_semantic"], eps=it.get("eps"), noise_seed=it.get("noise_seed"),
                             speed=it["speed"], **kw).cpu().numpy() for it in items]
    for it, s1 in zip(items, singles):
        assert s1.shape == (640 * e.vits_frames(it["pred_semantic"].size, it["speed"]),)
    e.set_option("seg_vocoder", 0)
    try:
        lanes = [o.cpu().numpy() for o in e.vits_decode_batch(items)]
        lanes_async = e.vits_decode_batch_async(items)
        e.vits_batch_wait()
    finally:
        e.set_option("seg_vocoder", 1)
    for i, s1 in enumerate(singles):
        np.testing.assert_array_equal(lanes[i], s1, err_msg=f"lanes, item {i}")
        np.testing.assert_array_equal(lanes_async[i].cpu().numpy(), s1, err_msg=f"async lanes, item {i}")
    n0 = e.counter("vits_packed_fronts")
    for sf in (0, 1):
        e.set_option("seg_front", sf)
        try:
            seg = [o.cpu().numpy() for o in e.vits_decode_batch(items)]
            seg_async = e.vits_decode_batch_async(items)
            e.vits_batch_wait()
        finally:
            e.set_option("seg_front", 1)
        for i, s1 in enumerate(singles):
            _close(seg[i], s1, f"seg_front {sf}, item {i}")
            np.testing.assert_array_equal(seg_async[i].cpu().numpy(), seg[i], err_msg=f"async, item {i}")
    assert e.counter("vits_packed_fronts") == n0                 # T' != T somewhere: not packed
    e.vits_decode_batch([dict(it, speed=1.0) for it in items[1:]])   # ... and all at speed 1: packed as before
    assert e.counter("vits_packed_fronts") == n0 + 1
    e.set_vocoder_cus(64)
    try:
        for it, s1 in zip(items, singles):
            audio = e.vits_decode_async(it)
            e.vits_wait()
            np.testing.assert_array_equal(audio.cpu().numpy(), s1)
    finally:
        e.set_vocoder_cus(0)


def test_philox_noise_at_speed(setup):
    """noise_seed at speed 0.8: the counter is the element index over 192 T' -- the oracle
    fed that stream (tests/philox.py) matches, and single and lane-batch calls are identical."""
    from tests.philox import vits_noise
    ver, e, vm, _ = setup
    G, S, seed, speed = 30, 20, 0xC0FFEE, 0.8
    txt, sem = _utt(G, S, "spp")
    kw = _cond(ver)
    frames = e.vits_frames(G, speed)
    eps = vits_noise(192 * frames, seed).reshape(1, 192, frames)
    ref = vits_oracle(vm, txt, sem, frames=frames, eps=eps, **kw).numpy()
    out = e.vits_decode(txt, sem, noise_seed=seed, speed=speed, **kw).cpu().numpy()
    _check_wave(out, ref, frames, "philox")
    other = dict(text_seq=txt, pred_semantic=sem, noise_seed=seed + 1, **kw)
    e.set_option("seg_vocoder", 0)
    try:
        batch = e.vits_decode_batch([dict(text_seq=txt, pred_semantic=sem, noise_seed=seed, speed=speed, **kw), other])
    finally:
        e.set_option("seg_vocoder", 1)
    np.testing.assert_array_equal(batch[0].cpu().numpy(), out)


def test_fp16_range_guard_reruns_f32_at_speed(setup):
    """test_vits_fp16_range_guard_reruns_f32's recipe (eps x 1e6) at speed 0.8: the re-run on
    the f32 path carries the speed -- 640 T' samples, equal bit for bit to the f32 path
    (convh 0) at that speed, which test_vits_waveform_conv_paths_at_odd_frames holds to the
    numpy oracle at ordinary amplitudes.  (At 1e6 x the noise the pre-tanh values are ~1e6 and
    an fp32 ulp there is ~0.1, so no RMS bound against a differently ordered CPU sum can be
    derived; the recipe's own reference, the f32 path, is the exact one.)"""
    ver, e, _, _ = setup
    G, S, speed = 24, 16, 0.8
    txt, sem = _utt(G, S, "spg")
    frames = e.vits_frames(G, speed)
    eps = (synth.rng_for(f"spbig{G}").standard_normal((1, 192, frames)) * 1e6).astype(np.float32)
    kw = _cond(ver)
    n0 = e.counter("vits_f32_reruns")
    out = e.vits_decode(txt, sem, eps=eps, speed=speed, **kw).cpu().numpy()
    assert e.counter("vits_f32_reruns") == n0 + 1
    e.set_option("convh", 0)
    try:
        ref = e.vits_decode(txt, sem, eps=eps, speed=speed, **kw).cpu().numpy()
    finally:
        e.set_option("convh", 1)
    assert out.shape == (640 * frames,) and np.isfinite(out).all()
    assert np.array_equal(out, ref)
    # the lanes' and the overlapped call's re-runs carry it too
    e.set_option("seg_vocoder", 0)
    try:
        it = dict(text_seq=txt, pred_semantic=sem, eps=eps, speed=speed, **kw)
        lanes = e.vits_decode_batch([it, dict(it, eps=eps * 1e-6)])
    finally:
        e.set_option("seg_vocoder", 1)
    assert e.counter("vits_f32_reruns") == n0 + 2
    assert np.array_equal(lanes[0].cpu().numpy(), ref)
    e.set_vocoder_cus(64)
    try:
        audio = e.vits_decode_async(it)
        e.vits_wait()
        assert np.array_equal(audio.cpu().numpy(), ref)
    finally:
        e.set_vocoder_cus(0)
    assert e.counter("vits_f32_reruns") == n0 + 3


def test_speed_is_validated(setup):
    from genie_tts_amd.engine import EngineError
    ver, e, _, _ = setup
    txt, sem = _utt(8, 10)
    kw = _cond(ver)
    for bad in (0.2, 4.5, float("nan")):
        with pytest.raises(ValueError):
            e.vits_decode(txt, sem, speed=bad, **kw)
    big = ((np.arange(1024, dtype=np.int64) * 37) % 1024).reshape(1, 1, -1)    # T' = 4097 at speed 0.5
    with pytest.raises(EngineError, match="too long"):
        e.vits_decode(txt, big, speed=0.5, **kw)


def test_api_tts_end_to_end_at_speed(monkeypatch):
    """api.tts(speed=1.25) on two sentences: the stream pipeline (vocoder_cus set, each
    sentence's vocoder item carrying the speed), 640 T'_i samples per sentence, equal to the
    oracle fed the engine's own tokens; speed 1.0 is the call without the argument, bit for bit."""
    import os
    import genie_tts_amd as G
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    from genie_tts_amd.model_manager import build_model, model_manager
    from oracle import restate as R
    from tests.test_api_gpu import GOLD, _eos_character
    div = np.load(os.path.join(GOLD, "pe_div_term.npy"))
    w = _eos_character()
    m = build_model(w, "v2", sampler=make_sampler(greedy=True), pe_div_term=div)
    m.VITS.noise = "zero"
    sp = m.T2S_FIRST_STAGE_DECODER.sampler
    try:
        model_manager._put("speed_char", m)
        model_manager.character_to_language["speed_char"] = "Japanese"
        ref = synth.synth_phones(12, "spe-r")
        ssl = synth.synth_ssl(41, "spe-s")
        audio32 = synth.synth_ref_audio(32000 * 2, "spe-a")
        G.set_reference_features("speed_char", ref, None, audio32, ssl)
        texts = [synth.synth_phones(10, "spe-t0"), synth.synth_phones(17, "spe-t1")]
        monkeypatch.setattr(api, "_sentences", lambda text, split: list(texts))
        seen = []
        real = m.ENGINE.vits_decode_async
        monkeypatch.setattr(m.ENGINE, "vits_decode_async",
                            lambda item, scale=0.5: (seen.append((item.get("speed"), m.ENGINE.vocoder_cus)),
                                                     real(item, scale))[1])
        out = G.tts("speed_char", None, sampler=sp, speed=1.25)
        assert seen == [(1.25, api.VOCODER_CUS)] * 2 and m.ENGINE.vocoder_cus == 0
        z = lambda n: np.zeros((n, 1024), np.float32)
        vm = R.VitsModel(w["vits"], "v2")
        want = []
        for t in texts:
            tok = m.ENGINE.t2s_generate([(ref, t, z(12), z(t.size), ssl.reshape(768, -1))], sp)[0]
            frames = m.ENGINE.vits_frames(tok.size, 1.25)
            want.append(vits_oracle(vm, t, tok.reshape(1, 1, -1), frames=frames, ref_audio=audio32).numpy())
            assert want[-1].shape == (640 * frames,)
        want = np.concatenate(want)
        assert out.shape == want.shape
        assert float(np.sqrt(np.mean((out - want) ** 2))) <= RMS_TOL
        plain = G.tts("speed_char", None, sampler=sp)
        assert np.array_equal(G.tts("speed_char", None, sampler=sp, speed=1.0), plain)
        assert plain.shape != out.shape
    finally:
        model_manager.character_to_model.pop("speed_char", None)
        api.clear_reference_audio_cache()
        m.ENGINE.close()
