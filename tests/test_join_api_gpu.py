"""GPU: the sentence join (`pause`, `trim`) from GENIE.tts / tts_stream / tts_batch, api.tts /
tts_async and the server's /tts down: each equals the same path's per-sentence vocoder output
put through the oracle (tests/trim_oracle.py) on the host -- bit-equal float32 at 32 kHz, and at
another rate Engine.audio_convert of the oracle's slice followed by the pause's zeros.

The runs that are compared decode on the per-step graphs (option "persist" 0), so which kernels a
run takes does not depend on the machine's load, and the engine's counters of
both runs are compared as tests/test_timbre_mix_gpu.py does."""
import asyncio
import os
import wave

import numpy as np
import pytest

from genie_tts_amd import synth
from tests import trim_oracle as O
from tests.test_timbre_mix_gpu import COUNTERS, NO_PERSIST

pytestmark = pytest.mark.gpu

PAUSE, TRIM = 0.3, -30.0


@pytest.fixture(scope="module")
def model():
    import genie_tts_amd as G
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    from genie_tts_amd.model_manager import build_model, model_manager
    from tests.test_api_gpu import GOLD, _eos_character
    div = np.load(os.path.join(GOLD, "pe_div_term.npy"))
    m = build_model(_eos_character(), "v2", sampler=make_sampler(greedy=True), pe_div_term=div)
    m.VITS.noise = "zero"
    m.ENGINE.set_option("persist", 0)
    model_manager._put("join_char", m)
    model_manager.character_to_language["join_char"] = "Japanese"
    G.set_reference_features("join_char", synth.synth_phones(12, "sra-r"), None,
                             synth.synth_ref_audio(32000 * 2, "sra-a"), synth.synth_ssl(41, "sra-s"))
    yield m
    model_manager.character_to_model.pop("join_char", None)
    api.clear_reference_audio_cache()
    m.ENGINE.close()


TEXTS = [synth.synth_phones(10, "sra-t0"), synth.synth_phones(17, "sra-t1")]


def _counted(m, fn):
    before = [m.ENGINE.counter(c) for c in COUNTERS]
    out = fn()
    return out, {c: m.ENGINE.counter(c) - b for c, b in zip(COUNTERS, before)}


def _same_kernels(what, sg, sw):
    print(f"{what}: counters {sg} against {sw}")
    same = [c for c in COUNTERS if c != "graph_fallbacks"]
    assert [sg[c] for c in same] == [sw[c] for c in same] and not any(sg[c] for c in NO_PERSIST), (what, sg, sw)


def _want(e, p, rate=32000, pcm=False, pause=PAUSE, trim=TRIM):
    """The sentence `p` (32 kHz float32, the path's plain output) joined on the host by the oracle."""
    p = np.asarray(p, np.float32).reshape(-1)
    if trim is not None:
        assert O.margin(p, trim) > 1e-6
    b, en = O.span(p, trim)
    y = e.audio_convert(p[b:en], rate, pcm16=pcm).cpu().numpy()
    if rate == 32000 and not pcm:
        assert np.array_equal(np.concatenate([y, np.zeros(O.pause_samples(rate, pause), np.float32)]),
                              O.join(p, pause, trim))
    return np.concatenate([y, np.zeros(O.pause_samples(rate, pause), y.dtype)])


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_genie_paths_equal_the_oracle_on_their_own_audio(model):
    from genie_tts_amd import api
    from genie_tts_amd.inference import GENIE
    m, e = model, model.ENGINE
    gen, sp = GENIE(), model.T2S_FIRST_STAGE_DECODER.sampler
    ref = api._reference_audios["join_char"]
    args = (ref, m.T2S_ENCODER, m.T2S_FIRST_STAGE_DECODER, m.T2S_STAGE_DECODER, m.VITS, m.PROMPT_ENCODER)
    variants = (dict(pause=PAUSE, trim=TRIM), dict(pause=PAUSE, trim=TRIM, sample_rate=48000, pcm16=True),
                dict(trim=TRIM, sample_rate=16000), dict(pause=PAUSE))

    def tts(**kw):
        return [gen.tts(t, *args, sampler=sp, **kw) for t in TEXTS]

    def stream(**kw):
        try:
            return list(gen.tts_stream(TEXTS, *args, sampler=sp, vocoder_cus=64, **kw))
        finally:
            e.set_vocoder_cus(0)

    def batch(**kw):
        return gen.tts_batch([(t, None) for t in TEXTS], ref, m, sp, **kw)

    for name, run in (("tts", tts), ("tts_stream", stream), ("tts_batch", batch)):
        plain, cp = _counted(m, run)
        assert len(plain) == 2 and all(p.dtype == np.float32 and p.size % 1280 == 0 and p.size for p in plain)
        for kw in variants:
            got, cg = _counted(m, lambda: run(**kw))
            _same_kernels(f"{name} {kw}", cg, cp)
            for p, g in zip(plain, got):
                want = _want(e, p, kw.get("sample_rate", 32000), kw.get("pcm16", False), kw.get("pause"),
                             kw.get("trim"))
                assert _eq(np.asarray(g).reshape(-1), want), (name, kw)
        again, _ = _counted(m, run)
        assert all(np.array_equal(a, p) for a, p in zip(again, plain)), name      # nothing moved
    # one value per item in the batch form
    plain = batch()
    got = batch(pause=[PAUSE, None], trim=[None, TRIM])
    assert _eq(got[0], _want(e, plain[0], trim=None)) and _eq(got[1], _want(e, plain[1], pause=None))
    with pytest.raises(ValueError):
        batch(pause=[PAUSE])
    with pytest.raises(ValueError):
        tts(trim=-10)


def test_api_tts_and_tts_async_join_each_sentence(model, monkeypatch, tmp_path):
    import genie_tts_amd as G
    from genie_tts_amd import api
    m, e = model, model.ENGINE
    sp = m.T2S_FIRST_STAGE_DECODER.sampler
    cur = []
    monkeypatch.setattr(api, "_sentences", lambda text, split: list(cur))
    singles = []
    for t in TEXTS:
        cur[:] = [t]
        singles.append(G.tts("join_char", None, sampler=sp))
    cur[:] = TEXTS
    plain = G.tts("join_char", None, sampler=sp)
    assert np.array_equal(plain, np.concatenate(singles))
    path = str(tmp_path / "joined.wav")
    got = G.tts("join_char", None, sampler=sp, pause=PAUSE, trim=TRIM, save_path=path)
    want = np.concatenate([_want(e, p) for p in singles])
    assert _eq(got, want) and got.size != plain.size
    with wave.open(path, "rb") as wf:                                 # the saved WAV includes the pauses
        assert wf.getframerate() == 32000 and wf.getnframes() == want.size
    got = G.tts("join_char", None, sampler=sp, pause=PAUSE, trim=TRIM, sample_rate=22050)
    assert _eq(got, np.concatenate([_want(e, p, 22050) for p in singles]))
    assert np.array_equal(G.tts("join_char", None, sampler=sp), plain)              # nothing moved

    async def go(**kw):
        return [c async for c in api.tts_async("join_char", None, sampler=sp, split_sentence=True, **kw)]
    assert asyncio.run(go(pause=PAUSE, trim=TRIM, sample_rate=48000)) == [
        _want(e, p, 48000, True).tobytes() for p in singles]
    from genie_tts_amd import audio as A
    assert asyncio.run(go(pause=PAUSE, trim=TRIM)) == [A.to_pcm16(_want(e, p)) for p in singles]
    assert asyncio.run(go()) == [A.to_pcm16(p) for p in singles]
    for bad in (dict(pause=-1), dict(trim=0), dict(pause=True)):
        with pytest.raises(ValueError):
            G.tts("join_char", None, sampler=sp, **bad)


def test_server_round_with_a_joined_and_a_plain_request(tmp_path):
    """test_sample_rate_gpu.py's server set-up: a request with pause and trim and one without, sent
    together.  The plain one is byte-equal to itself sent alone; the joined one is the plain one's
    PCM cut to the oracle's span (of the PCM's samples, every frame at least 1 % from the threshold)
    and followed by the pause's zeros.  A bad value is a 400."""
    import httpx
    from genie_tts_amd.server import Router, create_app
    wav = str(tmp_path / "ref.wav")
    x = (0.1 * np.random.default_rng(1).standard_normal(4 * 32000)).clip(-1, 1)
    with wave.open(wav, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(32000)
        wf.writeframes((x * 32767).astype("<i2").tobytes())
    text, G = "ありがとうございます。", 24

    async def run():
        router = Router([0], g2p="genie_tts_amd.stubs:toy_g2p", ssl="genie_tts_amd.stubs:toy_ssl", greedy=True,
                        noise="zero")
        router.start(asyncio.get_running_loop(), timeout=300)
        try:
            res = await router.broadcast("load_synthetic", character_name="srv", version="v2")
            assert all(r["kind"] == "ok" for r in res), res
            tr = httpx.ASGITransport(app=create_app(router))
            async with httpx.AsyncClient(transport=tr, base_url="http://t", timeout=300) as cl:
                r = await cl.post("/set_reference_audio", json=dict(character_name="srv", audio_path=wav,
                                                                    audio_text="こんにちは。", language="ja"))
                assert r.status_code == 200, r.text

                async def one(**kw):
                    r = await cl.post("/tts", json=dict(character_name="srv", text=text, force_steps=G + 1, **kw))
                    assert r.status_code == 200, r.text
                    return r
                alone = await one()
                joined, plain = await asyncio.gather(one(pause=PAUSE, trim=TRIM), one())
                bad = [await cl.post("/tts", json=dict(character_name="srv", text=text, **kw))
                       for kw in (dict(pause=5.5), dict(trim=-10.0), dict(trim=-90))]
                return alone, joined, plain, bad
        finally:
            router.close()
    alone, joined, plain, bad = asyncio.run(run())
    assert all(b.status_code == 400 and b.json()["detail"].startswith("join:") for b in bad)
    assert plain.content == alone.content and len(plain.content) == 2 * 1280 * G
    pcm = np.frombuffer(plain.content, np.int16)
    p = (pcm / 32767.0).astype(np.float32)
    assert O.margin(p, TRIM) > 1e-2
    b, en = O.span(p, TRIM)
    want = np.concatenate([pcm[b:en], np.zeros(O.pause_samples(32000, PAUSE), np.int16)])
    print(f"server: span [{b}, {en}) of {pcm.size} samples, {want.size} delivered")
    assert joined.content == want.tobytes()
