"""CPU: timbre fusion's host side (auxiliary reference clips, GPT-SoVITS's aux_ref_audio_paths)
-- engine.mix_weights (the one validation and normalisation point), ReferenceAudio.cond (the one
place the vocoder's conditioning is built; without auxiliary clips exactly what GENIE.tts,
tts_stream and tts_batch_vocoder built by hand), the per-clip and per-weights caches over a
stub engine, api.set_reference_audio's keywords and cache key, and the server's payload."""
import asyncio
import math

import numpy as np
import pytest


# ------------------------------------------------------------------ mix_weights
def test_mix_weights_none_is_the_plain_mean():
    from genie_tts_amd.engine import MIX_MAX, mix_weights
    for n in (1, 2, 3, 7, 16):
        w = mix_weights(n)
        assert w.dtype == np.float32 and w.shape == (n,)
        assert np.array_equal(w, np.full(n, np.float32(1.0 / n)))
    assert MIX_MAX == 16 and mix_weights(1, [5.0]).tolist() == [1.0]


def test_mix_weights_normalise_in_float64_round_once():
    from genie_tts_amd.engine import mix_weights
    w = mix_weights(3, [2, 1, 1])
    assert w.dtype == np.float32 and w.tolist() == [0.5, 0.25, 0.25]
    raw = [0.1, 0.7, 0.3, 1e-3]
    want = (np.array(raw, np.float64) / np.array(raw, np.float64).sum()).astype(np.float32)
    assert np.array_equal(mix_weights(4, raw), want)
    # float32 arithmetic gives other bits for some of these: the float64 path is what is specified
    f32 = np.array(raw, np.float32) / np.array(raw, np.float32).sum(dtype=np.float32)
    assert not np.array_equal(f32, want)
    assert np.array_equal(mix_weights(3, np.array([1, 0, 0], np.float32)), np.array([1, 0, 0], np.float32))
    assert np.array_equal(mix_weights(2, (np.float64(3), 1)), np.array([0.75, 0.25], np.float32))


@pytest.mark.parametrize("n, weights", [
    (3, [1.0, 1.0]), (2, [1.0, 1.0, 1.0]), (2, [[1.0, 1.0]]), (2, 1.0),          # wrong length / shape
    (2, [1.0, math.nan]), (2, [math.inf, 1.0]), (2, [1.0, -0.5]),                # non-finite, negative
    (2, [0.0, 0.0]),                                                             # zero sum
    (2, [True, 1.0]), (2, [1.0, np.bool_(False)]), (2, ["1", 1.0]),              # a bool, not a number
    (0, None), (17, None), (17, [1.0] * 17), (-1, None), (True, None), (2.0, None),   # n outside 1 .. 16
])
def test_mix_weights_rejections(n, weights):
    from genie_tts_amd.engine import mix_weights
    with pytest.raises(ValueError):
        mix_weights(n, weights)


# ------------------------------------------------------------------ ReferenceAudio.cond over a stub engine
class _StubEngine:
    """Stands in for Engine under the real sessions and GENIE driver.  A clip's ge is a constant
    vector holding its first sample, so a mix is checkable; every call is counted."""
    vocoder_cus = 0

    def __init__(self, G=6):
        self.G = G
        self.ref_encodes, self.prompt_encodes, self.mixes, self.projects, self.calls, self.t2s = [], [], [], [], [], []

    @staticmethod
    def vits_frames(n_sem, speed=1.0):
        from genie_tts_amd.engine import vits_frames
        return vits_frames(n_sem, speed)

    def t2s_generate(self, utts, sampler, **kw):
        self.t2s.append(utts)
        return [np.arange(self.G, dtype=np.int64) for _ in utts]

    def ref_encode(self, audio):
        a = np.asarray(audio, np.float32).reshape(-1)
        self.ref_encodes.append(float(a[0]))
        return np.full(512, a[0], np.float32)

    def prompt_encode(self, audio, sv_emb):
        a, sv = np.asarray(audio, np.float32).reshape(-1), np.asarray(sv_emb, np.float32).reshape(-1)
        self.prompt_encodes.append((float(a[0]), float(sv[0])))
        return np.full(1024, a[0] + sv[0], np.float32), np.full(512, -1.0, np.float32)

    def ge_mix(self, ges, weights):
        assert np.asarray(weights).dtype == np.float32
        self.mixes.append(np.asarray(weights).tolist())
        return sum(np.float32(w) * np.asarray(g, np.float32) for w, g in zip(weights, ges))

    def ge_project(self, ge):
        self.projects.append(1)
        return np.asarray(ge, np.float32)[:512] * np.float32(2)

    def vits_decode(self, text_seq, sem, speed=1.0, **kw):
        import torch
        self.calls.append(dict(kw, speed=speed))
        return torch.zeros(640 * self.vits_frames(np.asarray(sem).size, speed))


class _StubPromptEncoder:
    def __init__(self, engine):
        self.engine, self.runs = engine, 0

    def run(self, names, feed):
        self.runs += 1
        return [np.full((1, 1024, 1), 7.0, np.float32), np.full((1, 512, 1), 8.0, np.float32)]


def _clip(v, n=4096):
    return np.full((1, n), v, np.float32)


def _ref(**kw):
    from genie_tts_amd.inference import ReferenceAudio
    return ReferenceAudio(phonemes_seq=np.zeros((1, 4), np.int64), text_bert=np.zeros((4, 1024), np.float32),
                          audio_32k=_clip(1.0), ssl_content=np.zeros((1, 768, 8), np.float32), **kw)


@pytest.fixture
def fresh_caches():
    from genie_tts_amd import api
    api.clear_reference_audio_cache()
    yield api
    api.clear_reference_audio_cache()


def test_cond_without_aux_is_todays_dict(fresh_caches):
    from genie_tts_amd.sessions import VitsSession
    eng = _StubEngine()
    r = _ref()
    # V2, a vocoder that is not engine-backed: the clip itself
    other = type("Onnx", (), {})()
    c = r.cond(other)
    assert list(c) == ["ref_audio"] and c["ref_audio"] is r.audio_32k
    # V2, engine-backed: the session's v2_cond (ref_encode once per reference, then its ge)
    v = VitsSession(eng, "v2", noise="zero")
    c = r.cond(v)
    assert list(c) == ["ge"] and np.array_equal(c["ge"], np.full(512, 1.0, np.float32))
    assert r.cond(v)["ge"] is c["ge"] and eng.ref_encodes == [1.0]
    assert c["ge"] is v.v2_cond(r.audio_32k)["ge"]
    # V2ProPlus: update_global_emb's pair, cached after the first call
    pe = _StubPromptEncoder(eng)
    rp = _ref(sv_emb=np.zeros((1, 20480), np.float32))
    c = rp.cond(VitsSession(eng, "v2pp", noise="zero"), pe)
    assert list(c) == ["ge", "ge_advanced"] and c["ge"] is rp.global_emb and c["ge_advanced"] is rp.global_emb_advanced
    assert float(c["ge"][0, 0, 0]) == 7.0 and float(c["ge_advanced"][0, 0, 0]) == 8.0
    rp.cond(VitsSession(eng, "v2pp", noise="zero"), pe)
    assert pe.runs == 1
    with pytest.raises(ValueError, match="sv_emb"):
        _ref().cond(VitsSession(eng, "v2pp", noise="zero"), pe)
    assert eng.mixes == [] and eng.projects == [] and eng.prompt_encodes == []      # no mix ran at all


def test_cond_with_aux_encodes_each_clip_once_and_caches(fresh_caches):
    from genie_tts_amd.sessions import VitsSession
    eng = _StubEngine()
    v = VitsSession(eng, "v2", noise="zero")
    r = _ref(aux_audio_32k=[_clip(2.0), _clip(4.0)], weights=np.array([2, 1, 1]))
    c = r.cond(v)
    assert list(c) == ["ge"] and np.array_equal(c["ge"], np.full(512, 0.5 * 1 + 0.25 * 2 + 0.25 * 4, np.float32))
    assert eng.ref_encodes == [1.0, 2.0, 4.0] and eng.mixes == [[0.5, 0.25, 0.25]]
    assert r.cond(v)["ge"] is c["ge"] and len(eng.mixes) == 1                      # per (engine, weights)
    # the same clips in another reference with other weights: one more mix, nothing encoded again
    r2 = _ref(aux_audio_32k=[_clip(2.0), _clip(4.0)])
    c2 = r2.cond(v)
    third = float(np.float32(1.0 / 3))
    assert eng.ref_encodes == [1.0, 2.0, 4.0] and eng.mixes[1:] == [[third] * 3]
    assert not np.array_equal(c2["ge"], c["ge"])
    r.weights = [1, 0, 0]
    assert np.array_equal(r.cond(v)["ge"], np.full(512, 1.0, np.float32)) and len(eng.ref_encodes) == 3
    # another engine: its own embeddings
    eng_b = _StubEngine()
    r.cond(VitsSession(eng_b, "v2", noise="zero"))
    assert eng_b.ref_encodes == [1.0, 2.0, 4.0] and len(eng.ref_encodes) == 3
    # clear_reference_audio_cache forgets the per-clip embeddings
    fresh_caches.clear_reference_audio_cache()
    _ref(aux_audio_32k=[_clip(2.0), _clip(4.0)]).cond(v)
    assert eng.ref_encodes == [1.0, 2.0, 4.0] * 2
    # a vocoder that is not engine-backed cannot fuse; bad weights are mix_weights' ValueError
    with pytest.raises(ValueError, match="needs the engine"):
        r.cond(type("Onnx", (), {})())
    with pytest.raises(ValueError):
        _ref(aux_audio_32k=[_clip(2.0)], weights=[1.0, -1.0]).cond(v)
    with pytest.raises(ValueError):
        _ref(aux_audio_32k=[_clip(2.0)] * 16).cond(v)                               # 17 clips


def test_cond_v2proplus_uses_each_clips_sv_emb_and_projects_the_mix(fresh_caches):
    from genie_tts_amd.sessions import VitsSession
    eng = _StubEngine()
    v, pe = VitsSession(eng, "v2pp", noise="zero"), _StubPromptEncoder(eng)
    sv = lambda x: np.full((1, 20480), x, np.float32)
    r = _ref(sv_emb=sv(10), aux_audio_32k=[_clip(2.0), _clip(4.0)], aux_sv_emb=[sv(20), None],
             aux_audio_16k=[_clip(2.0, 2048), _clip(4.0, 2048)], weights=[0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match=r"sv_emb.*auxiliary clip 1"):              # today's error, naming the clip
        r.cond(v, pe)
    assert eng.prompt_encodes == [] and eng.mixes == []
    seen = []
    r.sv_fn = lambda a16: (seen.append(a16.shape), sv(30))[1]                       # as the primary's is obtained
    c = r.cond(v, pe)
    assert seen == [(1, 2048)] and eng.prompt_encodes == [(1.0, 10.0), (2.0, 20.0), (4.0, 30.0)]
    mix = 0.5 * 11 + 0.25 * 22 + 0.25 * 34
    assert list(c) == ["ge", "ge_advanced"] and np.array_equal(c["ge"], np.full(1024, mix, np.float32))
    assert np.array_equal(c["ge_advanced"], np.full(512, 2 * mix, np.float32))      # of the mix, not a mix of ge_adv
    assert pe.runs == 0 and eng.projects == [1]
    r.cond(v, pe)
    assert len(eng.mixes) == 1 and eng.projects == [1] and len(eng.prompt_encodes) == 3


def _stub_model(monkeypatch, eng, version="v2"):
    from types import SimpleNamespace
    from genie_tts_amd import api
    from genie_tts_amd.sessions import (EncoderSession, FirstStageDecoderSession, StageDecoderSession, VitsSession,
                                        _T2SState)
    st = _T2SState()
    m = SimpleNamespace(T2S_ENCODER=EncoderSession(eng), T2S_FIRST_STAGE_DECODER=FirstStageDecoderSession(eng, None, st),
                        T2S_STAGE_DECODER=StageDecoderSession(eng, None, st), VITS=VitsSession(eng, version, noise="zero"),
                        PROMPT_ENCODER=None, LANGUAGE="Japanese", ENGINE=eng)
    monkeypatch.setattr(api.model_manager, "get", lambda name: m)
    return api, m


def test_api_fused_reference_reaches_the_vocoder_and_t2s_sees_the_primary_only(monkeypatch, fresh_caches):
    eng = _StubEngine()
    api, m = _stub_model(monkeypatch, eng)
    ssl = np.full((1, 768, 8), 3.0, np.float32)
    api.set_reference_features("mx", [3, 5, 7], None, _clip(1.0), ssl, aux_audio_32k=[_clip(2.0), _clip(4.0)],
                               aux_weights=[0.5, 0.25, 0.25])
    txt = np.array([3, 5, 7], np.int64)
    assert api.tts("mx", txt).shape == (1280 * 6,)
    assert api.tts("mx", txt).shape == (1280 * 6,)
    assert eng.ref_encodes == [1.0, 2.0, 4.0] and len(eng.mixes) == 1               # once per reference set
    assert all(np.array_equal(c["ge"], np.full(512, 2.0, np.float32)) and c.get("ref_audio") is None
               for c in eng.calls) and len(eng.calls) == 2
    for utts in eng.t2s:                                                            # the primary's prompt alone
        assert np.asarray(utts[0][0]).tolist() == [[3, 5, 7]] and np.array_equal(utts[0][4], ssl[0])
    # the same clips with other weights: nothing is encoded again
    api.set_reference_features("mx", [3, 5, 7], None, _clip(1.0), ssl, aux_audio_32k=[_clip(2.0), _clip(4.0)])
    api.tts("mx", txt)
    assert eng.ref_encodes == [1.0, 2.0, 4.0] and len(eng.mixes) == 2
    # the batched path builds the same conditioning
    from genie_tts_amd.inference import tts_client
    seen = []
    eng.vits_decode_batch = lambda batch, scale: (seen.extend(batch), [0] * len(batch))[1]
    tts_client.tts_batch_vocoder([(txt, None)] * 2, [np.arange(6)] * 2, api._reference_audios["mx"], m)
    assert len(seen) == 2 and all(b["ge"] is seen[0]["ge"] and "ref_audio" not in b for b in seen)
    assert len(eng.mixes) == 2
    # back to the plain reference: the clip's own ge, no cached mix
    api.set_reference_features("mx", [3, 5, 7], None, _clip(1.0), ssl)
    api.tts("mx", txt)
    assert np.array_equal(eng.calls[-1]["ge"], np.full(512, 1.0, np.float32)) and len(eng.mixes) == 2
    with pytest.raises(ValueError):
        api.set_reference_features("mx", [3, 5, 7], None, _clip(1.0), ssl, aux_audio_32k=[_clip(2.0)],
                                   aux_weights=[1.0, 2.0, 3.0])


# ------------------------------------------------------------------ set_reference_audio
def test_set_reference_audio_aux_paths_cache_key_and_rejections(monkeypatch, tmp_path, fresh_caches):
    from genie_tts_amd import audio as A
    api = fresh_caches
    paths = []
    for i, secs in enumerate((3.0, 3.5, 4.0)):
        p = str(tmp_path / f"clip{i}.wav")
        A.write_wav(p, (0.1 * np.random.default_rng(i).standard_normal(int(secs * 32000))).astype(np.float32), 32000)
        paths.append(p)
    p0, p1, p2 = paths
    ssl, ps = np.zeros((1, 768, 20), np.float32), [3, 96, 222]
    hubert, g2p = [], []
    api.set_ssl_extractor(lambda a16: (hubert.append(a16.shape), ssl)[1])
    api.set_g2p(lambda text, lang: (g2p.append(text), (np.array([[3, 5]]), None))[1])
    try:
        api.set_reference_audio("a", p0, "t", "ja", phonemes_seq=ps, ssl_content=ssl)
        plain = api._reference_audios["a"]
        assert list(api._clip_cache) == [p0] and plain.aux_audio_32k == [] and plain.weights is None   # today's key
        api.set_reference_audio("a", p0, "t", "ja", aux_audio_paths=[p1, p2], aux_weights=[2, 1, 1])
        fused = api._reference_audios["a"]
        w = np.array([0.5, 0.25, 0.25], np.float32)
        assert fused is not plain and list(api._clip_cache) == [p0, (p0, (p1, p2), w.tobytes())]
        assert np.array_equal(fused.weights, w) and fused.weights.dtype == np.float32
        assert [a.shape for a in fused.aux_audio_32k] == [(1, int(3.5 * 32000) + 9600), (1, 4 * 32000 + 9600)]
        assert [a.shape[1] for a in fused.aux_audio_16k] == [a.shape[1] // 2 for a in fused.aux_audio_32k]
        assert np.array_equal(fused.audio_32k, plain.audio_32k)
        assert len(hubert) == 1 and g2p == ["t"]                     # CN-HuBERT and G2P: the primary only
        api.set_reference_audio("b", p0, "t", "ja", aux_audio_paths=[p1, p2], aux_weights=[4, 2, 2])
        assert api._reference_audios["b"] is fused                   # same normalised weights: the cached set
        api.set_reference_audio("b", p0, "t", "ja", aux_audio_paths=[p1, p2])
        assert api._reference_audios["b"] is not fused and len(api._clip_cache) == 3
        api.set_reference_audio("b", p0, "t", "ja")
        assert api._reference_audios["b"] is plain                   # the plain clip is still cached under its path
        # a bad auxiliary extension: logged, nothing changed
        before = (dict(api._reference_audios), list(api._clip_cache))
        api.set_reference_audio("a", p0, "t", "ja", aux_audio_paths=[p1, str(tmp_path / "x.mp3")])
        api.set_reference_audio("z", p0, "t", "ja", aux_audio_paths=[str(tmp_path / "x.mp3")])
        assert (dict(api._reference_audios), list(api._clip_cache)) == before
        # bad weights raise before a file is opened
        monkeypatch.setattr(A, "load_audio", lambda *a, **k: pytest.fail("a file was read"))
        for bad in ([1.0, 1.0], [1.0, -1.0, 1.0], [0, 0, 0], [1.0, math.nan, 1.0], [True, 1, 1]):
            with pytest.raises(ValueError):
                api.set_reference_audio("q", str(tmp_path / "new.wav"), "t", "ja", aux_audio_paths=[p1, p2],
                                        aux_weights=bad)
        with pytest.raises(ValueError):
            api.set_reference_audio("q", str(tmp_path / "new.wav"), "t", "ja",
                                    aux_audio_paths=[p1] * 16)        # 17 clips
        assert "q" not in api._reference_audios
    finally:
        api.set_ssl_extractor(None)
        api.set_g2p(None)


# ------------------------------------------------------------------ the server
def _echo_worker(index, conn, cfg):
    """Replies like _worker_main; a set_reference_audio is answered with an error that carries
    the broadcast fields, so the test reads what reached the worker."""
    conn.send(dict(kind="ready", id=-1, index=index))
    while True:
        msg = conn.recv()
        if msg is None:
            return
        if msg["cmd"] == "set_reference_audio":
            conn.send(dict(kind="error", id=msg["id"],
                           detail=repr((msg["audio_path"], msg["aux_audio_paths"], msg["aux_weights"]))))
        else:
            conn.send(dict(kind="ok", id=msg["id"]))


def test_server_payload_aux_fields():
    import httpx
    from genie_tts_amd.server import Router, create_app

    async def run():
        router = Router([0], worker=_echo_worker)
        router.start(asyncio.get_running_loop(), timeout=120)
        tr = httpx.ASGITransport(app=create_app(router))
        base = dict(character_name="a", audio_path="r.wav", audio_text="t", language="ja")
        try:
            async with httpx.AsyncClient(transport=tr, base_url="http://t") as cl:
                r = await cl.post("/set_reference_audio", json=base)
                assert r.status_code == 500 and r.json()["detail"] == repr(("r.wav", [], None))
                r = await cl.post("/set_reference_audio", json=dict(base, aux_audio_paths=["b.wav", "c.flac"],
                                                                    aux_weights=[2, 1, 1]))
                assert r.status_code == 500                          # the echo: both fields reached the worker
                assert r.json()["detail"] == repr(("r.wav", ["b.wav", "c.flac"], [2.0, 1.0, 1.0]))
                r = await cl.post("/set_reference_audio", json=dict(base, aux_audio_paths=["b.wav", "c.mp3"]))
                assert r.status_code == 400 and "mp3" in r.json()["detail"]
                for bad in ([1.0, 1.0], [1.0, -1.0, 1.0], [0, 0, 0]):
                    r = await cl.post("/set_reference_audio", json=dict(base, aux_audio_paths=["b.wav", "c.wav"],
                                                                        aux_weights=bad))
                    assert r.status_code == 400 and r.json()["detail"].startswith("aux_weights:"), bad
                r = await cl.post("/set_reference_audio", json=dict(base, aux_audio_paths=["b.wav"] * 16))
                assert r.status_code == 400
        finally:
            router.close()
    asyncio.run(run())


def test_aux_clips_as_one_array_and_unload_keeps_other_engines(monkeypatch, fresh_caches):
    """The auxiliary clips may be one 2-D array (a row per clip); unloading a character drops the
    embeddings and mixes on its engine only."""
    from types import SimpleNamespace
    from genie_tts_amd import inference
    from genie_tts_amd.sessions import VitsSession
    api = fresh_caches
    ssl = np.zeros((1, 768, 8), np.float32)
    api.set_reference_features("arr", [3, 5], None, _clip(1.0), ssl, aux_audio_32k=np.stack([_clip(2.0)[0], _clip(4.0)[0]]))
    ref = api._reference_audios["arr"]
    assert [a.shape for a in ref.aux_audio_32k] == [(1, 4096)] * 2 and ref.weights.tolist() == [np.float32(1 / 3)] * 3
    eng_a, eng_b = _StubEngine(), _StubEngine()
    ref.cond(VitsSession(eng_a, "v2", noise="zero"))
    ref.cond(VitsSession(eng_b, "v2", noise="zero"))
    assert len(inference._ge_cache) == 6 and len(ref._mix) == 2
    monkeypatch.setitem(api.model_manager.character_to_model, "gone", SimpleNamespace(ENGINE=eng_a))
    monkeypatch.setattr(api.model_manager, "remove_character", lambda name: None)
    api.unload_character("Gone")
    assert {k[0] for k in inference._ge_cache} == {id(eng_b)} and [k[0] for k in ref._mix] == [id(eng_b)]
    ref.cond(VitsSession(eng_b, "v2", noise="zero"))
    assert len(eng_b.ref_encodes) == 3                               # the other character encodes nothing again
    del eng_b, monkeypatch
    ref._mix.clear()
    import gc
    gc.collect()
    inference.clear_ge_cache(eng_a)                                  # entries of engines that are gone go too
    assert len(inference._ge_cache) == 0


def test_plain_v2_cond_on_another_engine_keeps_the_clip(fresh_caches):
    """tts_stream and tts_batch_vocoder name the model's engine: a plain V2 reference against a
    vocoder session backed by another engine is sent as `ref_audio`, as those sites did; a fused
    one is mixed on the vocoder's own engine."""
    from genie_tts_amd.sessions import VitsSession
    eng, other = _StubEngine(), _StubEngine()
    v = VitsSession(other, "v2", noise="zero")
    r = _ref()
    c = r.cond(v, None, eng)
    assert list(c) == ["ref_audio"] and c["ref_audio"] is r.audio_32k and other.ref_encodes == []
    assert list(r.cond(v, None, other)) == ["ge"] and list(r.cond(v)) == ["ge"]
    f = _ref(aux_audio_32k=[_clip(2.0)])
    assert list(f.cond(v, None, eng)) == ["ge"] and other.ref_encodes == [1.0, 1.0, 2.0] and eng.ref_encodes == []
