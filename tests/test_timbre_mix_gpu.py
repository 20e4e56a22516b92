"""GPU: timbre fusion (auxiliary reference clips; include/genie_engine.h, gsv_ge_mix and
gsv_ge_project) -- the mix kernel bit for bit against the numpy float32 chain, the projection
against gsv_prompt_encode's, the fused embedding and the waveform it gives against the CPU
oracle, and every synthesis path (GENIE.tts, tts_stream, tts_batch, api.tts) delivering the
audio of the same call made with the pre-mixed embedding passed explicitly.  Synthetic
characters, both model versions where they apply."""
from dataclasses import dataclass

import numpy as np
import pytest

from genie_tts_amd import synth
from genie_tts_amd.inference import ReferenceAudio
from tests import timbre_oracle as O
from tests.common import character

pytestmark = pytest.mark.gpu

WEIGHTS = (0.5, 0.25, 0.25)
RMS_TOL = 1e-4           # the project's parity limit
FORCE = 9                # forced decode steps (random weights never emit EOS)


@pytest.fixture(scope="module")
def clips():
    c0 = synth.synth_ref_audio(2 * 32000 + 1234, "ref")
    c1 = synth.synth_ref_audio(3 * 32000 + 77, "aux1")
    c2 = 3 * synth.synth_ref_audio(2 * 32000 + 4000, "aux2")
    assert c2.dtype == np.float32
    svs = [(0.1 * synth.rng_for(f"mix-sv{i}").standard_normal((1, 20480))).astype(np.float32) for i in range(3)]
    return [c0, c1, c2], svs


@pytest.fixture(scope="module", params=["v2", "v2ProPlus"])
def setup(request, clips):
    """One model per version, and the oracle's per-clip and fused embeddings, computed once."""
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler, mix_weights
    from genie_tts_amd.model_manager import build_model
    from oracle import restate as R
    ver = request.param
    w = character(ver)
    m = build_model(w, ver, sampler=make_sampler(greedy=True, force_steps=FORCE), vits_noise="zero")
    # These tests compare one synthesis run with another, bit for bit.  The persistent decode needs
    # all its workgroups resident; when other work on the device keeps a hand-off waiting past its
    # bound the engine runs the utterance again on the per-step graphs (and holds them for the next
    # generates), so which kernels a run takes would depend on the machine's load.  Timbre fusion
    # leaves T2S untouched, so every run here decodes on the per-step graphs, which need no
    # co-residency; the persistent decode has its own tests.
    m.ENGINE.set_option("persist", 0)
    vm = R.VitsModel(w["vits"], ver)
    cs, svs = clips
    ges = [O.clip_ge(w, vm, ver, c, sv) for c, sv in zip(cs, svs)]
    wts = mix_weights(3, WEIGHTS)
    yield dict(ver=ver, m=m, e=m.ENGINE, w=w, vm=vm, ges=ges, wts=wts, fused=O.fused(w, ver, ges, wts))
    api.clear_reference_audio_cache()
    m.ENGINE.close()


def _np(t):
    return t.float().cpu().numpy()


def _encode(s, clips):
    """Each clip's ge on the engine, the way ReferenceAudio.cond obtains it."""
    cs, svs = clips
    e = s["e"]
    return [e.ref_encode(c) if s["ver"] == "v2" else e.prompt_encode(c, sv)[0] for c, sv in zip(cs, svs)]


# ------------------------------------------------------------------ 1. the mix kernel
@pytest.mark.parametrize("dim, n", [(512, 3), (1024, 3), (513, 2), (513, 16), (1, 1), (1, 2), (512, 1), (1024, 16)])
def test_ge_mix_is_the_float32_chain(setup, dim, n):
    """dim 512 / 1024: the two models' sizes; 513: a one-thread tail block; 1: the smallest grid;
    n = 1, 2, 3 and GSV_MIX_MAX."""
    import torch
    from genie_tts_amd.engine import mix_weights
    e = setup["e"]
    r = synth.rng_for(f"mix{dim}x{n}")
    xs = [r.standard_normal(dim).astype(np.float32) for _ in range(n)]
    w = mix_weights(n, r.random(n) + 0.01)
    dev = [torch.as_tensor(x, device=e.dev) for x in xs]
    want = O.mix_chain_np(xs, w)
    got = _np(e.ge_mix(dev, w))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # out aliasing an input (the last, and the first)
    for k in {n - 1, 0}:
        cp = [d.clone() for d in dev]
        out = e.ge_mix(cp, w, out=cp[k])
        assert out.data_ptr() == cp[k].data_ptr() and np.array_equal(_np(out).view(np.uint32), want.view(np.uint32))
        assert all(np.array_equal(_np(c), x) for i, (c, x) in enumerate(zip(cp, xs)) if i != k)
    # weights (1, 0, ..): input 0 value for value
    one = np.zeros(n, np.float32)
    one[0] = 1.0
    assert np.array_equal(_np(e.ge_mix(dev, one)), xs[0])


def test_ge_mix_rejects_before_any_launch(setup):
    import torch
    from genie_tts_amd.engine import EngineError
    e = setup["e"]
    x = [torch.full((512,), float(i + 1), device=e.dev) for i in range(17)]
    out = torch.full((512,), -7.0, device=e.dev)
    eq = np.full(17, np.float32(1 / 17), np.float32)
    for ges, w, what in ((x, eq, "n outside"), (x[:2], [0.5, -0.5], "weight 1"), (x[:3], [0.5, 0.5, np.nan], "weight 2"),
                         (x[:2], [np.inf, 0.5], "weight 0"), (x[:2], [0.0, 0.0], "no weight above 0"),
                         ([], [], "n outside")):
        with pytest.raises(EngineError, match=what) as ei:
            e.ge_mix(ges, np.asarray(w, np.float32), out=out)
        assert "(-1)" in str(ei.value), ei.value                     # GSV_E_ARG
    empty = [torch.empty((0,), device=e.dev) for _ in range(2)]
    with pytest.raises(EngineError, match="dim outside"):
        e.ge_mix(empty, [0.5, 0.5], out=out)
    with pytest.raises(EngineError, match="dim outside"):
        e.ge_mix([torch.zeros(4097, device=e.dev)] * 2, [0.5, 0.5], out=torch.zeros(4097, device=e.dev))
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), np.full(512, -7.0, np.float32))  # nothing was launched


# ------------------------------------------------------------------ 2. the projection
def test_ge_project_is_prompt_encodes_last_step(setup, clips):
    from genie_tts_amd.engine import EngineError
    e, (cs, svs) = setup["e"], clips
    if setup["ver"] == "v2":
        with pytest.raises(EngineError, match="V2ProPlus"):
            e.ge_project(np.zeros(1024, np.float32))
        return
    ge, ga = e.prompt_encode(cs[0], svs[0])
    got = e.ge_project(ge)
    assert got.shape == (512,) and np.array_equal(_np(got).view(np.uint32), _np(ga).view(np.uint32))
    assert np.array_equal(_np(e.ge_project(_np(ge))), _np(ga))       # a host array in


# ------------------------------------------------------------------ 3. fused embedding against the oracle
def _fused_ref(s, clips, weights=WEIGHTS, cls=ReferenceAudio, **extra):
    """The test's reference: fused with `weights`, or (None) the primary clip alone."""
    cs, svs = clips
    v2 = s["ver"] == "v2"
    return cls(phonemes_seq=synth.synth_phones(12, "mix-r").reshape(1, -1), text_bert=np.zeros((12, 1024), np.float32),
               audio_32k=cs[0], ssl_content=synth.synth_ssl(41, "mix-s"), sv_emb=None if v2 else svs[0],
               aux_audio_32k=[] if weights is None else list(cs[1:]),
               aux_sv_emb=[] if v2 or weights is None else list(svs[1:]),
               weights=None if weights is None else np.asarray(weights), **extra)


def test_fused_embedding_against_the_oracle(setup, clips):
    """A convex combination's error is bounded by the largest per-clip error, so the fused
    embedding is held to the tolerance test_vits_gpu.py::test_prompt_encoder holds one clip to."""
    s = setup
    m = s["m"]
    c = _fused_ref(s, clips).cond(m.VITS, m.PROMPT_ENCODER)
    ge_o, adv_o = s["fused"]
    for i, (g, o) in enumerate(zip(_encode(s, clips), s["ges"])):
        print(f"{s['ver']} clip {i}: max |ge - oracle| {float(np.abs(_np(g) - o).max()):.3e}")
    print(f"{s['ver']} fused: max |ge - oracle| {float(np.abs(_np(c['ge']) - ge_o).max()):.3e}")
    assert sorted(c) == (["ge"] if s["ver"] == "v2" else ["ge", "ge_advanced"])
    np.testing.assert_allclose(_np(c["ge"]), ge_o, atol=2e-4, rtol=1e-4)
    if adv_o is not None:
        np.testing.assert_allclose(_np(c["ge_advanced"]), adv_o, atol=2e-4, rtol=1e-4)
    # and it is the chain over the engine's own per-clip embeddings, bit for bit
    want = O.mix_chain_np([_np(g) for g in _encode(s, clips)], s["wts"])
    assert np.array_equal(_np(c["ge"]).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ 4. waveform against the oracle
@pytest.mark.parametrize("G, S", [(8, 9), (20, 12)])
def test_fused_waveform_against_the_oracle(setup, G, S):
    s = setup
    e, ver = s["e"], s["ver"]
    txt = synth.synth_phones(S, f"mixw{S}")
    sem = ((np.arange(G, dtype=np.int64) * 37 + 11) % 1024).reshape(1, 1, G)
    ge, adv = s["fused"]
    ref = O.wave(s["vm"], ver, txt, sem, ge, adv)
    kw = dict(ge=ge) if ver == "v2" else dict(ge=ge, ge_advanced=adv)
    out = _np(e.vits_decode(txt, sem, **kw))                         # eps None, no seed: zero noise
    assert out.shape == (1280 * G,) == ref.shape
    rms = float(np.sqrt(np.mean((out - ref) ** 2)))
    ge0 = s["ges"][0]
    kw0 = dict(ge=ge0) if ver == "v2" else dict(ge=ge0, ge_advanced=O.project(s["w"], ge0))
    plain = _np(e.vits_decode(txt, sem, **kw0))
    apart = float(np.sqrt(np.mean((out - plain) ** 2)))
    print(f"{ver} G {G}: rms to the oracle {rms:.3e}, fused to primary-only {apart:.3e}")
    assert rms <= RMS_TOL, rms
    assert apart > 1e-2, apart                                       # the auxiliary clips are heard


# ------------------------------------------------------------------ 5. every synthesis path
@dataclass
class _Explicit(ReferenceAudio):
    """A reference whose conditioning is passed explicitly (`fixed`), or, without one, built the
    way GENIE.tts, tts_stream and tts_batch_vocoder built it before ReferenceAudio.cond."""
    fixed: dict = None

    def cond(self, vocoder, prompt_encoder=None, engine=None):
        if self.fixed is not None:
            return dict(self.fixed)
        if prompt_encoder is None:
            return vocoder.v2_cond(self.audio_32k)
        self.update_global_emb(prompt_encoder)
        return {"ge": self.global_emb, "ge_advanced": self.global_emb_advanced}


# What the engine counts of the kernels a run took: two runs are the same call only when these
# agree, and under the fixture's option "persist" 0 no persistent launch (so no hand-off timeout)
# may appear.  graph_fallbacks (a decode loop run eagerly after a failed capture: the same kernels)
# is printed only.
COUNTERS = ("persist_launches", "persist_timeouts", "persist1_f16_reruns", "vits_f32_reruns", "vits_packed_fronts",
            "lane_launches_0", "lane_launches_1", "graph_fallbacks")
NO_PERSIST = ("persist_launches", "persist_timeouts", "persist1_f16_reruns")


def _all_paths(m, ref):
    """The audio of GENIE.tts, a two-sentence tts_stream and a three-item tts_batch against ref,
    and what the engine's counters moved by meanwhile."""
    before = [m.ENGINE.counter(c) for c in COUNTERS]
    out = _run_paths(m, ref)
    return out, {c: m.ENGINE.counter(c) - b for c, b in zip(COUNTERS, before)}


def _run_paths(m, ref):
    from genie_tts_amd.inference import GENIE
    gen = GENIE()
    sp = m.T2S_FIRST_STAGE_DECODER.sampler
    texts = [synth.synth_phones(n, f"mix-t{n}") for n in (10, 13, 7)]
    args = (ref, m.T2S_ENCODER, m.T2S_FIRST_STAGE_DECODER, m.T2S_STAGE_DECODER, m.VITS, m.PROMPT_ENCODER)
    out = [gen.tts(texts[0], *args, sampler=sp)]
    try:
        out += list(gen.tts_stream(texts[:2], *args, sampler=sp, vocoder_cus=64))
    finally:
        m.ENGINE.set_vocoder_cus(0)
    out += gen.tts_batch([(t, None, FORCE) for t in texts], ref, m, sp)
    assert len(out) == 6 and all(o.ndim == 1 and o.size % 1280 == 0 and o.size > 0 for o in out)
    return out


PATHS = ("tts", "stream 0", "stream 1", "batch 0", "batch 1", "batch 2")


def _report(what, got, want):
    """Each path output against its counterpart, printed before anything is asserted; the two
    runs must have taken the same kernels, none of them the persistent decode's."""
    (got, sg), (want, sw) = got, want
    print(f"{what}: counters {sg} against {sw}")
    for name, a, b in zip(PATHS, got, want):
        d = np.abs(a - b) if a.shape == b.shape else None
        print(f"{what} {name}: " + ("shapes differ" if d is None else
                                      f"{int((d != 0).sum())} of {a.size} samples differ, max {float(d.max()):.3e}"))
    same = [c for c in COUNTERS if c != "graph_fallbacks"]
    assert [sg[c] for c in same] == [sw[c] for c in same] and not any(sg[c] for c in NO_PERSIST), (what, sg, sw)


def test_every_synthesis_path_delivers_the_fused_voice(setup, clips):
    from genie_tts_amd import api
    s = setup
    m, e = s["m"], s["e"]
    cs, svs = clips
    v2 = s["ver"] == "v2"
    # the pre-mixed conditioning, from the entries alone
    ge = e.ge_mix(_encode(s, clips), s["wts"])
    fixed = dict(ge=ge) if v2 else dict(ge=ge, ge_advanced=e.ge_project(ge))
    want = _all_paths(m, _fused_ref(s, clips, None, cls=_Explicit, fixed=fixed))
    api.set_reference_features("mixc", synth.synth_phones(12, "mix-r"), None, cs[0], synth.synth_ssl(41, "mix-s"),
                               sv_emb=None if v2 else svs[0], aux_audio_32k=cs[1:],
                               aux_sv_emb=None if v2 else svs[1:], aux_weights=WEIGHTS)
    got = _all_paths(m, api._reference_audios["mixc"])
    c = api._reference_audios["mixc"].cond(m.VITS, m.PROMPT_ENCODER)
    print(f"{s['ver']} conditioning equal to the pre-mixed one: " +
          ", ".join(f"{k} {np.array_equal(_np(c[k]), _np(fixed[k]))}" for k in fixed))
    assert all(np.array_equal(_np(c[k]).view(np.uint32), _np(fixed[k]).view(np.uint32)) for k in fixed)
    _report(s["ver"] + " fused", got, want)
    got, want = got[0], want[0]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), f"path output {i}"
    # a reference without auxiliary clips: today's bits, the conditioning built the old way
    plain_old = _all_paths(m, _fused_ref(s, clips, None, cls=_Explicit))
    plain = _all_paths(m, _fused_ref(s, clips, None))
    _report(s["ver"] + " plain", plain, plain_old)
    plain, plain_old = plain[0], plain_old[0]
    for i, (a, b) in enumerate(zip(plain, plain_old)):
        assert a.shape == b.shape and np.array_equal(a, b), f"plain path output {i}"
    assert all(float(np.sqrt(np.mean((a - b) ** 2))) > 1e-3 for a, b in zip(got, plain))


# ------------------------------------------------------------------ 6. api.tts end to end
def test_api_tts_fused_then_plain_leaks_no_mix(setup, clips):
    import genie_tts_amd as G
    from genie_tts_amd import api
    from genie_tts_amd.model_manager import model_manager
    s = setup
    m = s["m"]
    cs, svs = clips
    v2 = s["ver"] == "v2"
    assert m.VITS.noise == "zero"
    name = "mix_" + s["ver"].lower()
    model_manager.character_to_model[name] = m
    model_manager.character_to_language[name] = "Japanese"
    try:
        feats = (synth.synth_phones(12, "mix-r"), None, cs[0], synth.synth_ssl(41, "mix-s"))
        txt = synth.synth_phones(11, "mix-api")
        G.set_reference_features(name, *feats, sv_emb=None if v2 else svs[0])
        plain = G.tts(name, txt, split_sentence=False)
        G.set_reference_features(name, *feats, sv_emb=None if v2 else svs[0], aux_audio_32k=cs[1:],
                                 aux_sv_emb=None if v2 else svs[1:], aux_weights=WEIGHTS)
        fused = G.tts(name, txt, split_sentence=False)
        assert np.array_equal(fused, G.tts(name, txt, split_sentence=False))
        G.set_reference_features(name, *feats, sv_emb=None if v2 else svs[0])
        again = G.tts(name, txt, split_sentence=False)
        assert plain.shape == fused.shape == again.shape and plain.size > 0
        assert float(np.sqrt(np.mean((fused - plain) ** 2))) > 1e-3
        assert np.array_equal(again, plain)                          # no cached mix leaks
    finally:
        model_manager.character_to_model.pop(name, None)
        model_manager.character_to_language.pop(name, None)
        api.clear_reference_audio_cache()
