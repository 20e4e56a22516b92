"""GENIE inference driver (hot path), mirroring src/genie_tts/Core/Inference.py.

`GENIE.tts` has the reference's signature (Inference.py:16-61): it takes the
reference-audio features and the five sessions of a `GSVModel`, runs T2S, the
EOS filter and the vocoder, and returns `audio f32 [1280*G]` (`[640*T']` at a
speech rate `speed` other than 1, T' = Engine.vits_frames(G, speed)).  When the
sessions are this package's engine-backed ones (always, through
`model_manager`), T2S is one `gsv_t2s_generate` call: encoder, prefill, the
whole decode loop as one persistent kernel launch (per-step hipGraphs only as
the fp16-range / co-residency fallback), and the reference's trim + EOS filter
(Inference.py:41-44,108-109) -- no per-step host round trip.
`GENIE.t2s_cpu` is the reference's own session-by-session loop
(Inference.py:63-109) over the same sessions, kept for parity tests.

G2P (`get_phones_and_bert`, src/genie_tts/GetPhonesAndBert.py) is outside this
path: `tts` accepts phoneme ids (+ BERT features) directly, or text together
with a caller-supplied `g2p(text, language) -> (text_seq [1,S] i64, text_bert
[S,1024] f32)` -- e.g. the reference's own function.
"""
from __future__ import annotations

import threading
import weakref
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Union

import numpy as np

from .engine import (EngineStopped, Sampler, mix_weights, request_stop_all, vocoder_options,
                     vocoder_options_each)
from .sessions import (EncoderSession, FirstStageDecoderSession, StageDecoderSession, VitsSession,
                       PromptEncoderSession)

EOS = 1024
MAX_STEPS = 500          # Inference.py:95


# Per-clip global embeddings of fused references: (id(engine), V2ProPlus?, clip fingerprint) ->
# (weakref to the engine, ge on its device).  Shared by every ReferenceAudio, so the same clips
# set again with other weights encode nothing; dropped by clear_ge_cache().  api.tts_async and
# the replica threads may build a conditioning concurrently: every access holds _ge_lock.
_ge_cache: "OrderedDict[tuple, tuple]" = OrderedDict()
_ge_lock = threading.Lock()
GE_CACHE_MAX = 64


def clear_ge_cache(engine=None) -> None:
    """Forget the per-clip embeddings of fused references: all of them
    (api.clear_reference_audio_cache), or those on `engine` (api.unload_character) together with
    those of engines that are gone, whose device tensors the entries would otherwise keep."""
    with _ge_lock:
        if engine is None:
            _ge_cache.clear()
            return
        for key in [k for k, (ref, _) in _ge_cache.items() if ref() is None or ref() is engine]:
            del _ge_cache[key]


def _fingerprint(a) -> tuple:
    """A clip's content key, the one VitsSession.v2_cond uses: size, the float64 sum and 64 samples
    spread over the clip."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return a.size, float(a.sum(dtype=np.float64)), a[:: max(1, a.size // 64)].tobytes()


def _clip_ge(eng, audio_32k, sv_emb=None):
    """ge of one clip on `eng`, encoded once per (engine, clip): ref_encode (V2), or with the clip's
    sv_emb prompt_encode's ge (V2ProPlus)."""
    key = (id(eng), sv_emb is not None, _fingerprint(audio_32k), None if sv_emb is None else _fingerprint(sv_emb))
    with _ge_lock:
        hit = _ge_cache.get(key)
        if hit is not None and hit[0]() is eng:
            _ge_cache.move_to_end(key)
            return hit[1]
    a = np.ascontiguousarray(audio_32k, np.float32).reshape(-1)
    ge = eng.ref_encode(a) if sv_emb is None else eng.prompt_encode(a, np.asarray(sv_emb, np.float32).reshape(-1))[0]
    with _ge_lock:
        for k in [k for k, (ref, _) in _ge_cache.items() if ref() is None]:   # engines that are gone
            del _ge_cache[k]
        _ge_cache[key] = (weakref.ref(eng), ge)
        while len(_ge_cache) > GE_CACHE_MAX:
            _ge_cache.popitem(last=False)
    return ge


@dataclass
class ReferenceAudio:
    """Reference-audio features (the fields GENIE.tts reads from the reference's
    ReferenceAudio, src/genie_tts/Audio/ReferenceAudio.py:28-76).  api.set_reference_audio
    fills them from a clip: audio.py reads and resamples it (a polyphase restatement of
    soxr HQ), CN-HuBERT (gsv_hubert) gives ssl_content and, for V2ProPlus, the SV model
    (gsv_sv) gives sv_emb -- both on the engine; or the caller supplies them.

    Timbre fusion (GPT-SoVITS's aux_ref_audio_paths): aux_audio_32k holds further clips of the
    voice.  Each clip's global embedding is computed on its own by the same reference encoder
    and the vocoder is conditioned on ge = sum_i w_i ge_i, the primary clip first; `weights` is
    one weight per clip (engine.mix_weights: normalised to sum 1), None GPT-SoVITS's plain mean.
    On V2ProPlus every clip needs its own sv_emb (aux_sv_emb, or aux_audio_16k and an SV model),
    and ge_advanced is ge_to512 of the mixed ge.  The prompt of T2S -- phonemes_seq, text_bert,
    ssl_content -- is the primary clip's alone: auxiliary clips need no text and run neither G2P
    nor CN-HuBERT.  cond() is the one place the vocoder's conditioning is built."""
    phonemes_seq: np.ndarray             # i64 [1, R]
    text_bert: np.ndarray                # f32 [R, 1024]
    audio_32k: np.ndarray                # f32 [1, N32]
    ssl_content: np.ndarray              # f32 [1, 768, H]
    sv_emb: Optional[np.ndarray] = None  # f32 [1, 20480] (V2ProPlus)
    global_emb: Optional[np.ndarray] = None
    global_emb_advanced: Optional[np.ndarray] = None
    text: str = ""
    audio_16k: Optional[np.ndarray] = None               # f32 [1, N16] (set_reference_audio)
    sv_fn: Optional[Callable] = None                     # speaker-verification model, audio_16k -> sv_emb
    aux_audio_32k: list = field(default_factory=list)    # auxiliary clips, f32 [1, N32] each
    aux_audio_16k: list = field(default_factory=list)    # their 16 kHz copies (V2ProPlus: for the SV model)
    aux_sv_emb: list = field(default_factory=list)       # their sv_emb f32 [1, 20480] (None: from the SV model)
    weights: Optional[np.ndarray] = None                 # one per clip, primary first (None: equal)
    # the fused conditioning: (id(engine), V2ProPlus?, float32 weights) -> (weakref to the engine, dict)
    _mix: dict = field(default_factory=dict, repr=False, compare=False)

    def update_global_emb(self, prompt_encoder) -> None:
        """ReferenceAudio.py:68-76 (cached after the first call)."""
        if self.global_emb is not None:
            return
        if self.sv_emb is None and self.sv_fn is not None and self.audio_16k is not None:
            self.sv_emb = np.asarray(self.sv_fn(self.audio_16k), np.float32).reshape(1, -1)
        if self.sv_emb is None:
            raise ValueError("V2ProPlus needs the speaker-verification embedding (sv_emb) of the reference: "
                             "load_sv_model(), set_sv_extractor() or pass sv_emb")
        self.global_emb, self.global_emb_advanced = prompt_encoder.run(None, {
            "ref_audio": self.audio_32k, "sv_emb": self.sv_emb})

    def aux_sv(self, i: int) -> np.ndarray:
        """sv_emb of auxiliary clip i (V2ProPlus), obtained like the primary's: given, else sv_fn
        on its 16 kHz copy (kept).  ValueError naming the clip when there is neither."""
        while len(self.aux_sv_emb) < len(self.aux_audio_32k):
            self.aux_sv_emb.append(None)
        if self.aux_sv_emb[i] is None and self.sv_fn is not None and i < len(self.aux_audio_16k) \
                and self.aux_audio_16k[i] is not None:
            self.aux_sv_emb[i] = np.asarray(self.sv_fn(self.aux_audio_16k[i]), np.float32).reshape(1, -1)
        if self.aux_sv_emb[i] is None:
            raise ValueError("V2ProPlus needs the speaker-verification embedding (sv_emb) of the reference: "
                             f"load_sv_model(), set_sv_extractor() or pass sv_emb (auxiliary clip {i})")
        return self.aux_sv_emb[i]

    def drop_engine(self, engine) -> None:
        """Forget the fused conditioning cached for `engine` (api.unload_character)."""
        with _ge_lock:
            for key in [k for k in self._mix if k[0] == id(engine)]:
                del self._mix[key]

    def reset_cond(self) -> None:
        """Forget the cached conditioning (an sv_emb was replaced)."""
        self.global_emb = self.global_emb_advanced = None
        with _ge_lock:
            self._mix.clear()

    def cond(self, vocoder, prompt_encoder=None, engine=None) -> dict:
        """The conditioning keys of a vocoder call against this reference, the one place they
        are built (GENIE.tts, tts_stream and tts_batch_vocoder call it).
        Without auxiliary clips, today's: V2 `ref_audio` for a vocoder that is not engine-backed
        (or, when the caller names its `engine`, not backed by that one), else the session's
        v2_cond (gsv_ref_encode once per reference, then its ge); V2ProPlus update_global_emb's
        ge / ge_advanced.  No mix runs.
        With auxiliary clips: every clip's ge once per (engine, clip) (_clip_ge), their mix
        (Engine.ge_mix) and, on V2ProPlus, its projection (Engine.ge_project) once per (engine,
        weights), as device tensors; later calls are a dictionary look-up.  ValueError for a
        vocoder that is not engine-backed, bad weights, or a V2ProPlus clip without sv_emb."""
        eng = getattr(vocoder, "engine", None)
        backed = eng is not None and hasattr(vocoder, "v2_cond")
        if not getattr(self, "aux_audio_32k", None):
            if prompt_encoder is None:
                own = backed and (engine is None or eng is engine)
                return vocoder.v2_cond(self.audio_32k) if own else {"ref_audio": self.audio_32k}
            self.update_global_emb(prompt_encoder)
            return {"ge": self.global_emb, "ge_advanced": self.global_emb_advanced}
        if not backed:
            raise ValueError("timbre fusion (auxiliary reference clips) needs the engine: the vocoder session "
                             "is not engine-backed")
        w = mix_weights(1 + len(self.aux_audio_32k), self.weights)
        v2pp = prompt_encoder is not None
        key = (id(eng), v2pp, w.tobytes())
        with _ge_lock:
            hit = self._mix.get(key)
        if hit is not None and hit[0]() is eng:
            return dict(hit[1])
        if v2pp:
            if self.sv_emb is None and self.sv_fn is not None and self.audio_16k is not None:
                self.sv_emb = np.asarray(self.sv_fn(self.audio_16k), np.float32).reshape(1, -1)
            if self.sv_emb is None:
                raise ValueError("V2ProPlus needs the speaker-verification embedding (sv_emb) of the reference: "
                                 "load_sv_model(), set_sv_extractor() or pass sv_emb")
            svs = [self.sv_emb] + [self.aux_sv(i) for i in range(len(self.aux_audio_32k))]
        else:
            svs = [None] * (1 + len(self.aux_audio_32k))
        ges = [_clip_ge(eng, a, sv) for a, sv in zip([self.audio_32k, *self.aux_audio_32k], svs)]
        out = {"ge": eng.ge_mix(ges, w)}
        if v2pp:
            out["ge_advanced"] = eng.ge_project(out["ge"])
        with _ge_lock:
            self._mix[key] = (weakref.ref(eng), out)
        return dict(out)


def _cond(ref, vocoder, prompt_encoder, engine=None) -> dict:
    """ref.cond(vocoder, prompt_encoder, engine).  A stand-in that only carries the fields GENIE.tts
    reads (no auxiliary clips) is served by ReferenceAudio.cond all the same."""
    fn = getattr(ref, "cond", None)
    return (fn(vocoder, prompt_encoder, engine) if fn is not None
            else ReferenceAudio.cond(ref, vocoder, prompt_encoder, engine))


def eos_filter(semantic_tokens: np.ndarray) -> np.ndarray:
    """Inference.py:41-44: cut at the first id >= 1024."""
    idx = np.where(semantic_tokens >= EOS)
    if len(idx[0]) > 0:
        semantic_tokens = semantic_tokens[..., :idx[-1][0]]
    return semantic_tokens


def _engine_of(*sessions):
    engines = {id(getattr(s, "engine", None)) for s in sessions}
    if len(engines) == 1 and all(isinstance(s, (EncoderSession, FirstStageDecoderSession, StageDecoderSession,
                                                VitsSession)) for s in sessions):
        return sessions[0].engine
    return None


class StopEvent(threading.Event):
    """GENIE.stop_event (Inference.py:13-14): a threading.Event whose set()/clear() also
    set/clear the stop word of every engine (gsv_request_stop), so a decode running on
    the device leaves within two loop steps, as the reference's per-step check
    (Inference.py:96-97) does."""

    def set(self):
        super().set()
        request_stop_all(True)

    def clear(self):
        super().clear()
        request_stop_all(False)


class GENIE:
    def __init__(self):
        self.stop_event = StopEvent()

    def tts(self, text: Union[str, np.ndarray], prompt_audio: ReferenceAudio, encoder, first_stage_decoder,
            stage_decoder, vocoder, prompt_encoder=None, language: str = "japanese",
            text_bert: Optional[np.ndarray] = None, g2p: Optional[Callable] = None,
            sampler: Optional[Sampler] = None, speed: float = 1.0, sample_rate: Optional[int] = None,
            pcm16: bool = False, loudness: Optional[float] = None,
            peak: Optional[float] = None, pause: Optional[float] = None,
            trim: Optional[float] = None) -> Optional[np.ndarray]:
        """speed, sample_rate / pcm16, loudness / peak, pause / trim: engine.vocoder_options
        (ValueError for a bad value, before any GPU work); none given: the reference's audio."""
        rate = vocoder_options(speed, sample_rate, pcm16, loudness, peak, pause, trim)
        if isinstance(text, str):
            if g2p is None:
                raise ValueError("text input needs a g2p(text, language) callable (G2P is outside this engine)")
            text_seq, text_bert = g2p("。" + text, language)          # Inference.py:27-28
        else:
            text_seq = np.asarray(text, np.int64).reshape(1, -1)
            if text_bert is None:
                text_bert = np.zeros((text_seq.shape[1], 1024), np.float32)
        eng = _engine_of(encoder, first_stage_decoder, stage_decoder, vocoder)
        if eng is not None:
            sem = self.t2s(prompt_audio.phonemes_seq, prompt_audio.text_bert, text_seq, text_bert,
                           prompt_audio.ssl_content, eng, sampler or first_stage_decoder.sampler)
            if sem is None:            # stopped (Inference.py:96-97)
                return None
        else:
            sem = self.t2s_cpu(prompt_audio.phonemes_seq, prompt_audio.text_bert, text_seq, text_bert,
                               prompt_audio.ssl_content, encoder, first_stage_decoder, stage_decoder)
            if sem is None:
                return None
            sem = eos_filter(sem)
        return vocoder.run(None, {"text_seq": text_seq, "pred_semantic": sem,
                                  **_cond(prompt_audio, vocoder, prompt_encoder), **rate})[0]

    def tts_stream(self, texts: Sequence[Union[str, np.ndarray]], prompt_audio: ReferenceAudio, encoder,
                   first_stage_decoder, stage_decoder, vocoder, prompt_encoder=None, language: str = "japanese",
                   text_bert: Optional[np.ndarray] = None, g2p: Optional[Callable] = None,
                   sampler: Optional[Sampler] = None, vocoder_cus: int = 64, speed: float = 1.0,
                   sample_rate: Optional[int] = None, pcm16: bool = False, loudness: Optional[float] = None,
                   peak: Optional[float] = None, pause: Optional[float] = None, trim: Optional[float] = None):
        """tts over a list of sentences, yielding each sentence's audio in order (the
        reference runs them one after the other: TTSPlayer._tts_worker_loop,
        Core/TTSPlayer.py:56-107).  Engine-backed sessions pipeline them: sentence i's
        vocoder runs on `vocoder_cus` CUs of its own while sentence i+1's T2S runs on
        the rest (gsv_vits_decode_async), and sentence i+1's encoder + prefill run on
        those CUs during sentence i's decode (gsv_t2s_prefetch), so sentence i is
        yielded once sentence i+1's T2S is done.  Same tokens and audio as calling
        tts per sentence.  speed, sample_rate / pcm16, loudness / peak: as for tts, of every
        sentence on its own; the output stage and the measurement run on the vocoder's CUs too.
        pause / trim: every sentence, the last included, is cut to its speech and followed by its
        pause on the GPU; the yielded array has the joined length."""
        opts = vocoder_options(speed, sample_rate, pcm16, loudness, peak, pause, trim)   # a bad value fails before anything starts
        speed = opts.pop("speed", 1.0)
        eng = _engine_of(encoder, first_stage_decoder, stage_decoder, vocoder)
        if eng is None or vocoder_cus <= 0 or len(texts) < 2:
            for t in texts:
                if self.stop_event.is_set():
                    return
                yield self.tts(t, prompt_audio, encoder, first_stage_decoder, stage_decoder, vocoder, prompt_encoder,
                               language, text_bert, g2p, sampler, speed, **opts)
            return
        prev_cus = eng.vocoder_cus     # restored when the stream ends: later single-sentence and
        if prev_cus != vocoder_cus:    # batched calls keep every CU (decode groups, lanes)
            eng.set_vocoder_cus(vocoder_cus)
        try:
            cond = _cond(prompt_audio, vocoder, prompt_encoder, eng)
        except BaseException:          # e.g. a V2ProPlus clip without sv_emb: the CU split is undone
            if eng.vocoder_cus != prev_cus:
                eng.set_vocoder_cus(prev_cus)
            raise
        # every sentence's inputs up front: sentence i+1's T2S is queued behind sentence
        # i's, its encoder + prefill run on the vocoder CUs while sentence i decodes
        seqs = []
        for t in texts:
            if isinstance(t, str):
                if g2p is None:
                    raise ValueError("text input needs a g2p(text, language) callable (G2P is outside this engine)")
                seqs.append(g2p("。" + t, language))
            else:
                ts = np.asarray(t, np.int64).reshape(1, -1)
                seqs.append((ts, text_bert if text_bert is not None else np.zeros((ts.shape[1], 1024), np.float32)))
        ssl = np.asarray(prompt_audio.ssl_content, np.float32).reshape(768, -1)
        utts = [(prompt_audio.phonemes_seq, ts, prompt_audio.text_bert, tb, ssl) for ts, tb in seqs]
        sp = sampler or first_stage_decoder.sampler
        pending = None
        n = len(utts)
        try:
            eng.t2s_prefetch(utts[1], sp)          # launched beside sentence 0's decode
            eng.t2s_generate_start(utts[0], sp)
            for i, (text_seq, _) in enumerate(seqs):
                if self.stop_event.is_set():
                    break
                if i + 1 < n:                      # queued behind sentence i's decode
                    if i + 2 < n:
                        eng.t2s_prefetch(utts[i + 2], sp)
                    eng.t2s_generate_start(utts[i + 1], sp)
                try:
                    sem = eng.t2s_generate_finish().reshape(1, 1, -1)
                except EngineStopped:          # stop_event during sentence i's decode
                    break
                if pending is not None:
                    eng.vits_wait()
                    done, pending = eng.vits_joined([pending])[0], None
                    yield done.cpu().numpy()
                G = sem.size
                eps = vocoder.eps(G, speed)
                item = dict(text_seq=text_seq, pred_semantic=sem, speed=speed, **cond, **opts)
                if eps is not None:
                    item["eps"] = eps
                else:
                    seed = vocoder.next_seed()
                    if seed is not None:
                        item["noise_seed"] = seed
                pending = eng.vits_decode_async(item, vocoder.noise_scale)
            if pending is not None:
                eng.vits_wait()
                done, pending = eng.vits_joined([pending])[0], None
                yield done.cpu().numpy()
        finally:   # stopped, failed or abandoned: started generates and the vocoder call complete
            while getattr(eng, "_gq", None):
                try:
                    eng.t2s_generate_finish()
                except Exception:
                    break
            if pending is not None:
                eng.vits_wait()
            if eng.vocoder_cus != prev_cus:
                eng.set_vocoder_cus(prev_cus)

    def t2s(self, ref_seq, ref_bert, text_seq, text_bert, ssl_content, engine,
            sampler: Sampler) -> Optional[np.ndarray]:
        """Whole T2S on the device; returns the trimmed, EOS-filtered [1,1,G] tokens, or
        None when stop_event interrupted it (Inference.py:96-97)."""
        try:
            tok = engine.t2s_generate([(ref_seq, text_seq, ref_bert, text_bert,
                                        np.asarray(ssl_content, np.float32).reshape(768, -1))], sampler)[0]
        except EngineStopped:
            return None
        return tok.reshape(1, 1, -1)

    def t2s_cpu(self, ref_seq, ref_bert, text_seq, text_bert, ssl_content, encoder, first_stage_decoder,
                stage_decoder) -> Optional[np.ndarray]:
        """The reference's loop (Inference.py:63-109) over session objects."""
        x, prompts = encoder.run(None, {"ref_seq": ref_seq, "text_seq": text_seq, "ref_bert": ref_bert,
                                        "text_bert": text_bert, "ssl_content": ssl_content})
        y, y_emb, *present = first_stage_decoder.run(None, {"x": x, "prompts": prompts})
        names: List[str] = [i.name for i in stage_decoder.get_inputs()]
        idx = 0
        for idx in range(0, MAX_STEPS):
            if self.stop_event.is_set():
                return None
            outs = stage_decoder.run(None, dict(zip(names, [y, y_emb, *present])))
            y, y_emb, stop, *present = outs
            if stop:
                break
        y[0, -1] = 0
        return np.expand_dims(y[:, -idx:], axis=0)

    def tts_batch(self, items: Sequence[tuple], prompt_audio: ReferenceAudio, model, sampler: Sampler,
                  speed: Union[float, Sequence[float]] = 1.0, samplers: Optional[Sequence[Sampler]] = None,
                  streams: Optional[Sequence[int]] = None, sample_rate=None, pcm16=False, loudness=None,
                  peak=None, pause=None, trim=None) -> List[np.ndarray]:
        """Batched synthesis for one character and reference: items are
        (text_seq, text_bert|None[, force_steps]).  All sequences decode together
        (one multi-sequence persistent launch, ragged: a finished sequence drops out);
        the vocoder runs each utterance's text/flow part on concurrent lanes and the
        generator once over the whole batch (gsv_vits_decode_batch).  samplers / streams: one
        sampler (and Philox stream) per item instead of `sampler`, still one launch
        (Engine.t2s_generate).  speed, sample_rate / pcm16, loudness / peak, pause / trim: one
        value for all items or one per item (tts_batch_vocoder)."""
        toks = (self.tts_batch_t2s(items, prompt_audio, model, sampler) if samplers is None and streams is None
                else self.tts_batch_t2s(items, prompt_audio, model, sampler, samplers=samplers, streams=streams))
        wavs = self.tts_batch_vocoder(items, toks, prompt_audio, model, speed=speed, sample_rate=sample_rate,
                                      pcm16=pcm16, loudness=loudness, peak=peak, pause=pause, trim=trim)
        return [w if isinstance(w, np.ndarray) else w.cpu().numpy() for w in wavs]

    def tts_batch_t2s(self, items: Sequence[tuple], prompt_audio: ReferenceAudio, model, sampler: Sampler,
                      samplers: Optional[Sequence[Sampler]] = None, streams: Optional[Sequence[int]] = None):
        """The T2S half of tts_batch: one ragged batched generate -> token arrays.  samplers:
        one per item, used instead of `sampler`; streams: their Philox stream words."""
        ssl = np.asarray(prompt_audio.ssl_content, np.float32).reshape(768, -1)
        utts = [(prompt_audio.phonemes_seq, it[0], prompt_audio.text_bert, it[1], ssl,
                 it[2] if len(it) > 2 else 0) for it in items]
        # one generate for the whole batch: the engine's multi-sequence persistent decode
        # (B <= 64) costs ~2 ms per extra sequence over a single one
        # (profiles/r03i_batch_sweep.json), so splitting never pays
        if samplers is None and streams is None:
            return model.ENGINE.t2s_generate(utts, sampler)
        return model.ENGINE.t2s_generate(utts, None, samplers=samplers, streams=streams)

    def tts_batch_vocoder(self, items: Sequence[tuple], toks, prompt_audio: ReferenceAudio, model,
                          overlapped: bool = False, speed: Union[float, Sequence[float]] = 1.0,
                          sample_rate=None, pcm16=False, loudness=None, peak=None, pause=None, trim=None):
        """The vocoder half of tts_batch.  overlapped=True (engine-backed vocoder only) starts
        the batch on the vocoder lanes and returns device tensors that are valid after
        model.ENGINE.vits_batch_wait(); the T2S of the next batch runs beside it
        (gsv_vits_decode_batch_async).  speed, sample_rate / pcm16, loudness / peak
        (engine.vocoder_options): one value or one per item (None entries: that item as ever).  A
        batch may mix them: one launch of the engine's output stage converts the whole batch, and
        the items with a target are measured in one pass and their gains applied by that launch.
        pause / trim: the same way; overlapped, the tensors hold the longest a sentence can get and
        model.ENGINE.vits_joined(them) cuts them to their joined lengths after the wait."""
        eng = model.ENGINE
        opts = vocoder_options_each(len(items), speed, sample_rate, pcm16, loudness, peak, pause, trim)   # before any GPU work
        cond = _cond(prompt_audio, model.VITS, model.PROMPT_ENCODER, eng)   # the reference branch once per reference
        if getattr(model.VITS, "engine", None) is not eng:
            return [model.VITS.run(None, {"text_seq": it[0], "pred_semantic": tok.reshape(1, 1, -1), **cond, **o})[0]
                    for it, tok, o in zip(items, toks, opts)]
        # engine-backed vocoder: all utterances on concurrent lanes (gsv_vits_decode_batch)
        batch = [dict(text_seq=it[0], pred_semantic=tok, noise_seed=model.VITS.next_seed(), **cond, **o)
                 for it, tok, o in zip(items, toks, opts)]
        if overlapped:
            return eng.vits_decode_batch_async(batch, model.VITS.noise_scale)
        return eng.vits_decode_batch(batch, model.VITS.noise_scale)


tts_client = GENIE()
