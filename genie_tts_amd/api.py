"""The `genie_tts` entry points this engine serves (src/genie_tts/__init__.py:1-28,
src/genie_tts/Internal.py:94-330), restricted to the synthesis hot path.

Same names, argument meaning and defaults as the reference:
  load_character(character_name, onnx_model_dir, language)        Internal.py:94-126
  set_reference_audio(character_name, audio_path, audio_text, language=None)
                                                                   Internal.py:143-190
  tts(character_name, text, play=False, split_sentence=True, save_path=None)
                                                                   Internal.py:265-310
  tts_async(character_name, text, play=False, split_sentence=False, save_path=None)
      -> async iterator of 16-bit PCM bytes, one chunk per sentence Internal.py:193-262
  unload_character, clear_reference_audio_cache, stop, wait_for_playback_done

What the engine does not contain (outside the hot path) is pluggable:
  set_g2p(fn(text, language) -> (phones i64 [1,S], bert f32 [S,1024]))   -- G2P (+ BERT), or
          -> (phones, None, input_ids, word2ph): RoBERTa then runs on the engine (load_roberta)
  set_ssl_extractor(fn(audio_16k [1,N]) -> ssl_content [1,768,H])       -- CN-HuBERT override
  set_sv_extractor(fn(audio_16k [1,N]) -> sv_emb [1,20480])             -- V2ProPlus SV model
CN-HuBERT itself runs on the engine (gsv_hubert) once load_cn_hubert(dir | weights) has
been called or $HUBERT_MODEL_DIR is set (ModelManager.py:172-195),
or the features can be passed to set_reference_audio directly (phonemes_seq=,
text_bert=, ssl_content=, sv_emb=).  Reading/resampling the clip is audio.py
(own WAV/AIFF reader + polyphase resampler: soundfile/soxr are absent).
Differences: `tts` also returns the audio; `play=True` has no output device in
this environment and is skipped with a warning, as the reference does when
sounddevice fails (Core/TTSPlayer.py:136-146).
"""
from __future__ import annotations

import asyncio
import functools
import logging
import os
import threading
from collections import OrderedDict
from typing import AsyncIterator, Callable, Dict, List, Optional, Sequence, Union

import numpy as np

from . import audio as A
from .engine import mix_weights, vocoder_options
from .inference import ReferenceAudio, clear_ge_cache, tts_client
from .model_manager import model_manager
from .text_splitter import TextSplitter

logger = logging.getLogger(__name__)

SAMPLE_RATE = 32000
# CUs reserved for the overlapped vocoder of multi-sentence synthesis (0: sequential)
VOCODER_CUS = int(os.environ.get("GENIE_VOCODER_CUS", "64"))
SUPPORTED_AUDIO_EXTS = A.SUPPORTED_AUDIO_EXTS
_reference_audios: Dict[str, ReferenceAudio] = {}
_clip_cache: "OrderedDict[str, ReferenceAudio]" = OrderedDict()   # ReferenceAudio._prompt_cache (LRU 10)
_g2p: Optional[Callable] = None
_ssl_extractor: Optional[Callable] = None
_sv_extractor: Optional[Callable] = None
# The player's session stop (TTSPlayer._stop_event, Core/TTSPlayer.py:208-222): set by stop(),
# cleared when a tts / tts_async session starts (TTSPlayer.start_session, :175).  A stopped
# session synthesizes no further sentence and saves nothing; tts_client.stop_event (GENIE's)
# is the per-sentence word that abandons a running decode, cleared per sentence as the
# worker loop does (:86).
_session_stop = threading.Event()


def _norm_language(language: Optional[str]) -> str:
    if language is None:
        return "Japanese"
    l = language.lower()
    return {"ja": "Japanese", "jp": "Japanese", "japanese": "Japanese", "en": "English", "english": "English",
            "zh": "Chinese", "chinese": "Chinese", "hybrid": "Hybrid-Chinese-English",
            "hybrid-chinese-english": "Hybrid-Chinese-English"}.get(l, language)


def set_g2p(fn: Optional[Callable]) -> None:
    """fn(text, language) -> (text_seq i64 [1,S], text_bert f32 [S,1024])."""
    global _g2p
    _g2p = fn


def set_ssl_extractor(fn: Optional[Callable]) -> None:
    """fn(audio_16k f32 [1,N]) -> ssl_content f32 [1,768,H] (the reference's CN-HuBERT session)."""
    global _ssl_extractor
    _ssl_extractor = fn


def load_cn_hubert(model=None) -> None:
    """CN-HuBERT weights: the GenieData/chinese-hubert-base directory or a dict of
    arrays (weights.hubert_spec names); `g/ModelManager.py:172-195`."""
    model_manager.load_cn_hubert(model)


def load_roberta(model=None) -> None:
    """RoBERTa (chinese-roberta-wwm-ext-large) weights: the GenieData RoBERTa directory
    or a dict of arrays (weights.roberta_spec names); `g/ModelManager.py:132-150`."""
    model_manager.load_roberta_model(model)


def load_sv_model(model=None) -> None:
    """Speaker-verification weights (V2ProPlus sv_emb): GenieData speaker_encoder.onnx
    (or its directory) or a dict of arrays (weights.sv_spec names); runs on the engine
    (gsv_sv).  `g/ModelManager.py:155-170`."""
    model_manager.load_sv_model(model)


def set_sv_extractor(fn: Optional[Callable]) -> None:
    """fn(audio_16k f32 [1,N]) -> sv_emb f32 [1,20480] (the reference's speaker-verification session)."""
    global _sv_extractor
    _sv_extractor = fn


def load_character(character_name: str, onnx_model_dir: Union[str, os.PathLike], language: str) -> None:
    """Internal.py:94-126: load a converted character directory."""
    language = _norm_language(language)
    if language not in ("Japanese", "English", "Chinese", "Hybrid-Chinese-English"):
        raise ValueError("Unknown language")
    model_manager.load_character(character_name, os.fspath(onnx_model_dir), language)


def load_weights(character_name: str, weights, version: str, language: str = "Japanese") -> None:
    """Register a character from in-memory weights (e.g. genie_tts_amd.synth)."""
    model_manager.load_weights(character_name, weights, version, _norm_language(language))


def unload_character(character_name: str) -> None:
    m = model_manager.character_to_model.get(character_name.lower())
    eng = getattr(m, "ENGINE", None)
    model_manager.remove_character(character_name)
    if eng is None:
        return
    # fused references: this character's per-clip embeddings and mixes live on its engine and go
    # with it; other characters' stay cached
    clear_ge_cache(eng)
    for ref in list(_reference_audios.values()) + list(_clip_cache.values()):
        if isinstance(ref, ReferenceAudio):
            ref.drop_engine(eng)


def _text_features(text: str, language: str, phonemes_seq=None, text_bert=None):
    if phonemes_seq is None:
        if _g2p is None:
            raise ValueError("no G2P: pass phonemes_seq (and text_bert) or call set_g2p()")
        g = _g2p(text, language)
        phonemes_seq, text_bert = g[0], g[1]
        if len(g) == 4 and text_bert is None and model_manager.roberta is not None:
            # (phones, None, input_ids, word2ph): Chinese BERT features on the engine
            # (GetPhonesAndBert.py:64-74; tokenizing text_clean stays with the G2P)
            ids = np.asarray(g[2], np.int64).reshape(1, -1)
            text_bert = model_manager.roberta.run(None, {"input_ids": ids, "attention_mask": np.ones_like(ids),
                                                         "repeats": np.asarray(g[3], np.int64)})[0]
    ps = np.asarray(phonemes_seq, np.int64).reshape(1, -1)
    tb = np.zeros((ps.shape[1], 1024), np.float32) if text_bert is None else np.asarray(text_bert, np.float32)
    return ps, tb


def _check_ext(path: str) -> bool:
    ext = os.path.splitext(path)[1].lower()
    if ext not in SUPPORTED_AUDIO_EXTS:
        logger.error("Audio format '%s' is not supported. Only the following formats are supported: %s", ext,
                     sorted(SUPPORTED_AUDIO_EXTS))
        return False
    return True


def _sv_list(aux_sv_emb, n: int) -> list:
    """aux_sv_emb as one entry per auxiliary clip (None: from the SV model)."""
    if aux_sv_emb is None:
        return [None] * n
    if len(aux_sv_emb) != n:
        raise ValueError(f"aux_sv_emb: one per auxiliary clip ({n}), None where the SV model supplies it")
    return [None if e is None else np.asarray(e, np.float32).reshape(1, -1) for e in aux_sv_emb]


def set_reference_audio(character_name: str, audio_path: Union[str, os.PathLike], audio_text: str,
                        language: Optional[str] = None, *, phonemes_seq=None, text_bert=None,
                        ssl_content=None, sv_emb=None, aux_audio_paths=None, aux_weights=None,
                        aux_sv_emb=None) -> None:
    """Internal.py:143-190 + ReferenceAudio.py:28-57: the clip at 32 kHz (+0.3 s
    silence) and 16 kHz, the prompt text's phones/BERT, the SSL content of the 16 kHz
    clip; cached per clip path (LRU, Max_Cached_Reference_Audio).
    aux_audio_paths: auxiliary clips whose timbre is fused with the primary's (GPT-SoVITS's
    aux_ref_audio_paths; inference.ReferenceAudio), read like the primary -- same formats, same
    duration warning -- and needing no text.  aux_weights: one weight per clip, primary first
    (engine.mix_weights; None: the plain mean), checked before any file is read (ValueError).
    aux_sv_emb (V2ProPlus): one per auxiliary clip, None where the SV model supplies it.  With
    auxiliary clips the cache key is (path, aux paths, weights)."""
    path = os.fspath(audio_path)
    aux_paths = [] if aux_audio_paths is None else [os.fspath(p) for p in aux_audio_paths]
    weights = mix_weights(1 + len(aux_paths), aux_weights) if aux_paths or aux_weights is not None else None
    aux_sv = _sv_list(aux_sv_emb, len(aux_paths))
    if not all([_check_ext(p) for p in [path, *aux_paths]]):
        return
    if language is None:
        m = model_manager.get(character_name)
        if m is None:
            raise ValueError("No language specified")
        language = m.LANGUAGE
    language = _norm_language(language)
    if language not in ("Japanese", "English", "Chinese"):
        raise ValueError("Unknown language")
    key = (path, tuple(aux_paths), weights.tobytes()) if aux_paths else path
    ref = _clip_cache.get(key)
    if ref is None:
        audio_32k = A.load_audio(path, 32000).reshape(1, -1)
        audio_16k = A.resample(audio_32k[0], 32000, 16000).reshape(1, -1)
        aux_32k = [A.load_audio(p, 32000).reshape(1, -1) for p in aux_paths]
        aux_16k = [A.resample(a[0], 32000, 16000).reshape(1, -1) for a in aux_32k]   # V2ProPlus: for the SV model
        if ssl_content is None:
            if _ssl_extractor is not None:
                ssl_content = _ssl_extractor(audio_16k)
            elif model_manager.cn_hubert is not None or os.getenv("HUBERT_MODEL_DIR"):
                model_manager.load_cn_hubert()          # ReferenceAudio.py:48-52
                ssl_content = model_manager.cn_hubert.run(None, {"input_values": audio_16k})[0]
            else:
                raise ValueError("no SSL extractor (CN-HuBERT): load_cn_hubert(), pass ssl_content "
                                 "or call set_ssl_extractor()")
        ps, tb = _text_features(audio_text, language, phonemes_seq, text_bert)
        ref = ReferenceAudio(phonemes_seq=ps, text_bert=tb, audio_32k=audio_32k,
                             ssl_content=np.asarray(ssl_content, np.float32).reshape(1, 768, -1),
                             sv_emb=None if sv_emb is None else np.asarray(sv_emb, np.float32).reshape(1, -1),
                             text=audio_text, aux_audio_32k=aux_32k, aux_audio_16k=aux_16k, aux_sv_emb=aux_sv,
                             weights=weights if aux_paths else None)
        ref.audio_16k = audio_16k
        ref.sv_fn = _sv_extractor
        _clip_cache[key] = ref
        while len(_clip_cache) > int(os.getenv("Max_Cached_Reference_Audio", "10")):
            _clip_cache.popitem(last=False)
    else:
        _clip_cache.move_to_end(key)
        if ref.text != audio_text or phonemes_seq is not None:      # ReferenceAudio.py:18-21 set_text
            ref.phonemes_seq, ref.text_bert = _text_features(audio_text, language, phonemes_seq, text_bert)
            ref.text = audio_text
        if sv_emb is not None:
            ref.sv_emb = np.asarray(sv_emb, np.float32).reshape(1, -1)
            ref.reset_cond()
        if any(e is not None for e in aux_sv):
            ref.aux_sv_emb = [new if new is not None else old for new, old in
                              zip(aux_sv, list(ref.aux_sv_emb) + [None] * len(aux_sv))]
            ref.reset_cond()
    _reference_audios[character_name] = ref


def set_reference_features(character_name: str, phonemes_seq: np.ndarray, text_bert: Optional[np.ndarray],
                           audio_32k: np.ndarray, ssl_content: np.ndarray, sv_emb: Optional[np.ndarray] = None,
                           audio_text: str = "", aux_audio_32k=None, aux_sv_emb=None, aux_weights=None) -> None:
    """Set the reference from already-extracted features (the fields GENIE.tts reads).
    aux_audio_32k: auxiliary clips (32 kHz float32 arrays) whose timbre is fused with the
    primary's, aux_weights their weights, primary first (engine.mix_weights; None: the plain
    mean), aux_sv_emb (V2ProPlus) one sv_emb per auxiliary clip, None where the SV model supplies
    it: inference.ReferenceAudio.  ValueError for bad weights."""
    aux = [] if aux_audio_32k is None else [np.asarray(a, np.float32).reshape(1, -1) for a in aux_audio_32k]
    weights = mix_weights(1 + len(aux), aux_weights) if aux or aux_weights is not None else None
    ps = np.asarray(phonemes_seq, np.int64).reshape(1, -1)
    tb = np.zeros((ps.shape[1], 1024), np.float32) if text_bert is None else np.asarray(text_bert, np.float32)
    _reference_audios[character_name] = ReferenceAudio(
        phonemes_seq=ps, text_bert=tb, audio_32k=np.asarray(audio_32k, np.float32).reshape(1, -1),
        ssl_content=np.asarray(ssl_content, np.float32).reshape(1, 768, -1),
        sv_emb=None if sv_emb is None else np.asarray(sv_emb, np.float32).reshape(1, -1), text=audio_text,
        aux_audio_32k=aux, aux_sv_emb=_sv_list(aux_sv_emb, len(aux)), weights=weights if aux else None)


def clear_reference_audio_cache() -> None:
    _reference_audios.clear()
    _clip_cache.clear()
    clear_ge_cache()                 # the per-clip embeddings of fused references


def _sentences(text, split_sentence: bool) -> List:
    if isinstance(text, str):
        return TextSplitter().split(text.strip()) if split_sentence else ([text] if text else [])
    return [np.asarray(text, np.int64)]               # phoneme ids: one utterance


def _ensure_sv_emb(m, ref) -> None:
    """V2ProPlus: the reference clip's speaker embedding, once per clip
    (ReferenceAudio.update_global_emb, `g/Audio/ReferenceAudio.py:68-76`): a plugged
    extractor, else the engine's SV model (load_sv_model() or $SV_MODEL_PATH)."""
    if m.PROMPT_ENCODER is None:
        return
    _ensure_aux_sv_emb(ref)
    if ref.sv_emb is not None:
        return
    if getattr(ref, "sv_fn", None) is not None:
        ref.sv_emb = np.asarray(ref.sv_fn(ref.audio_16k), np.float32).reshape(1, -1)
    elif getattr(ref, "audio_16k", None) is not None and (model_manager.speaker_verification_model is not None
                                                          or os.getenv("SV_MODEL_PATH")):
        model_manager.load_sv_model()
        sv = model_manager.speaker_verification_model.run(None, {"waveform": ref.audio_16k})[0]
        ref.sv_emb = np.asarray(sv, np.float32).reshape(1, -1)


def _ensure_aux_sv_emb(ref) -> None:
    """The auxiliary clips' speaker embeddings, obtained like the primary's, once per clip: a
    plugged extractor (ReferenceAudio.aux_sv), else the engine's SV model on the clip's 16 kHz
    copy (made here for a reference set from arrays).  A clip left without one fails in
    ReferenceAudio.cond, which names it."""
    aux = getattr(ref, "aux_audio_32k", None) or []
    if not aux:
        return
    ref.aux_sv_emb = (list(ref.aux_sv_emb) + [None] * len(aux))[:len(aux)]
    ref.aux_audio_16k = (list(ref.aux_audio_16k) + [None] * len(aux))[:len(aux)]
    have_sv = model_manager.speaker_verification_model is not None or bool(os.getenv("SV_MODEL_PATH"))
    for i, a in enumerate(aux):
        if ref.aux_sv_emb[i] is not None or (ref.sv_fn is None and not have_sv):
            continue
        if ref.aux_audio_16k[i] is None:
            ref.aux_audio_16k[i] = A.resample(np.asarray(a, np.float32).reshape(-1), 32000, 16000).reshape(1, -1)
        if ref.sv_fn is not None:
            ref.aux_sv(i)
        else:
            model_manager.load_sv_model()
            sv = model_manager.speaker_verification_model.run(None, {"waveform": ref.aux_audio_16k[i]})[0]
            ref.aux_sv_emb[i] = np.asarray(sv, np.float32).reshape(1, -1)


def _sampling(top_k=None, top_p=None, temperature=None, repetition_penalty=None, seed=None) -> dict:
    """The sampling keywords of a synthesis call that were given, validated (ValueError for
    a value the engine rejects) before anything is synthesized."""
    from .engine import check_sampling
    return check_sampling(top_k=top_k, top_p=top_p, temperature=temperature,
                          repetition_penalty=repetition_penalty, seed=seed)


def _resolve_sampler(character_name: str, sampler, fields: dict):
    """The sampler of a call: `sampler` as passed when no keyword overrides a field (today's
    call, unchanged), else a copy of it -- or of the character's own -- with those fields set."""
    if not fields:
        return sampler
    from .engine import override_sampler
    if sampler is None:
        m = model_manager.get(character_name)
        if m is None:
            raise ValueError(f"character '{character_name}' is not loaded")
        sampler = m.T2S_FIRST_STAGE_DECODER.sampler
    return override_sampler(sampler, **fields)


def _synthesize(character_name: str, sentence, text_bert=None, sampler=None, **opts) -> np.ndarray:
    """One sentence; opts: the call's engine.vocoder_options."""
    m = model_manager.get(character_name)
    if m is None:
        raise ValueError(f"character '{character_name}' is not loaded")
    ref = _reference_audios[character_name]
    _ensure_sv_emb(m, ref)
    if _session_stop.is_set():
        return None
    tts_client.stop_event.clear()            # TTSPlayer.py:86, per sentence
    if _session_stop.is_set():               # a stop() between the check and the clear
        tts_client.stop_event.set()
        return None
    return tts_client.tts(sentence, ref, m.T2S_ENCODER, m.T2S_FIRST_STAGE_DECODER, m.T2S_STAGE_DECODER, m.VITS,
                          m.PROMPT_ENCODER, m.LANGUAGE, text_bert=text_bert, g2p=_g2p, sampler=sampler,
                          **opts)


def _synthesize_all(character_name: str, sentences: List, text_bert=None, sampler=None, **opts):
    """Every sentence, in order; on the engine the vocoder of one sentence overlaps the
    T2S of the next (GENIE.tts_stream)."""
    if len(sentences) < 2:
        return [_synthesize(character_name, s, text_bert, sampler, **opts) for s in sentences]
    m = model_manager.get(character_name)
    if m is None:
        raise ValueError(f"character '{character_name}' is not loaded")
    ref = _reference_audios[character_name]
    _ensure_sv_emb(m, ref)
    if _session_stop.is_set():
        return []
    tts_client.stop_event.clear()
    if _session_stop.is_set():
        tts_client.stop_event.set()
        return []
    return list(tts_client.tts_stream(sentences, ref, m.T2S_ENCODER, m.T2S_FIRST_STAGE_DECODER, m.T2S_STAGE_DECODER,
                                      m.VITS, m.PROMPT_ENCODER, m.LANGUAGE, text_bert=text_bert, g2p=_g2p,
                                      sampler=sampler, vocoder_cus=VOCODER_CUS, **opts))


def _play(audio: np.ndarray, sample_rate: int = SAMPLE_RATE) -> None:
    try:
        import sounddevice as sd   # noqa: F401  (absent here, as on most servers)
        sd.play(np.asarray(audio, np.float32).squeeze(), sample_rate)
        sd.wait()
    except Exception as e:      # TTSPlayer.py:136-146: playback skipped, synthesis goes on
        logger.warning("Failed to initialize sounddevice: %s. Audio playback will be skipped.", e)


def _write_pcm16_wav(path: str, pcm: bytes, sample_rate: int) -> None:
    """A 16-bit mono WAV from samples that are already int16 (the GPU's output stage)."""
    import wave
    parent = os.path.dirname(path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(sample_rate)
        wf.writeframes(pcm)


def tts(character_name: str, text: Union[str, Sequence[int], np.ndarray], play: bool = False,
        split_sentence: bool = True, save_path: Union[str, os.PathLike, None] = None,
        text_bert: Optional[np.ndarray] = None, sampler=None, speed: float = 1.0, *,
        top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: Optional[float] = None,
        repetition_penalty: Optional[float] = None, seed: Optional[int] = None,
        sample_rate: Optional[int] = None, loudness: Optional[float] = None,
        peak: Optional[float] = None, pause: Optional[float] = None,
        trim: Optional[float] = None) -> Optional[np.ndarray]:
    """Internal.py:265-310 (TTSPlayer session: split, synthesize each sentence, save the
    concatenation as 16-bit WAV).  Returns the audio f32 [sum 1280*G_i] at 32 kHz.
    speed, sample_rate, loudness / peak: engine.vocoder_options, per sentence (ValueError for a
    bad value, before anything is synthesized).  The audio is returned, saved (the WAV header
    carries the rate) and played at sample_rate, as float32.
    pause, trim: the sentence join, per sentence on the GPU (engine.vocoder_options): each sentence
    is cut to its speech above `trim` dBFS and followed by `pause` seconds of silence, the last
    included (GPT-SoVITS's fragment_interval); the returned and the saved audio include the pauses.
    top_k (1..64), top_p (0 < p <= 1, nucleus sampling), temperature (> 0), repetition_penalty
    (> 0), seed: GPT-SoVITS's sampling controls; None keeps the field of `sampler` (or, without
    one, of the character's sampler), a value overrides it on a copy.  ValueError for a bad value."""
    opts = vocoder_options(speed, sample_rate, False, loudness, peak, pause, trim)
    out_rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
    fields = _sampling(top_k, top_p, temperature, repetition_penalty, seed)
    if character_name not in _reference_audios:
        logger.error("Please call 'set_reference_audio' first to set the reference audio.")
        return None
    sampler = _resolve_sampler(character_name, sampler, fields)
    _session_stop.clear()                    # TTSPlayer.start_session
    chunks = [c for c in _synthesize_all(character_name, _sentences(text, split_sentence), text_bert, sampler,
                                         **opts)
              if c is not None]
    audio = np.concatenate(chunks) if chunks else np.zeros(0, np.float32)
    if _session_stop.is_set():               # stopped: the session's STREAM_END (and its save) never runs
        return audio
    if save_path:
        A.write_wav(os.fspath(save_path), audio, out_rate)
    if play:
        _play(audio, out_rate)
    return audio


async def tts_async(character_name: str, text: str, play: bool = False, split_sentence: bool = False,
                    save_path: Union[str, os.PathLike, None] = None, speed: float = 1.0, *, sampler=None,
                    top_k: Optional[int] = None, top_p: Optional[float] = None,
                    temperature: Optional[float] = None, repetition_penalty: Optional[float] = None,
                    seed: Optional[int] = None, sample_rate: Optional[int] = None,
                    loudness: Optional[float] = None, peak: Optional[float] = None,
                    pause: Optional[float] = None, trim: Optional[float] = None) -> AsyncIterator[bytes]:
    """Internal.py:193-262: yields one raw 16-bit PCM chunk per sentence as soon as it
    is synthesized (TTSPlayer chunk callback), the engine running off the event loop.
    speed, sampler, the sampling keywords, sample_rate, loudness / peak and pause / trim: as for
    tts (a chunk is a joined sentence, its pause included).  With a
    sample_rate the chunks are the int16 samples at that rate as the GPU's output stage wrote
    them (32000 gives the bytes of the call without it); None: converted on the host."""
    opts = vocoder_options(speed, sample_rate, sample_rate is not None, loudness, peak, pause, trim)
    out_rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
    fields = _sampling(top_k, top_p, temperature, repetition_penalty, seed)
    if character_name not in _reference_audios:
        raise ValueError("Please call 'set_reference_audio' first to set the reference audio.")
    sampler = _resolve_sampler(character_name, sampler, fields)
    loop = asyncio.get_running_loop()
    _session_stop.clear()                    # TTSPlayer.start_session
    chunks = []
    for s in _sentences(text, split_sentence):
        if _session_stop.is_set():
            return
        audio = await loop.run_in_executor(None, functools.partial(_synthesize, character_name, s, sampler=sampler,
                                                                     **opts))
        if _session_stop.is_set():
            # stop() during the sentence: the reference's worker sends chunk_callback(None) and
            # the iterator ends without that chunk (TTSPlayer.py:109-114, Internal.py:258-262)
            return
        if audio is None:
            continue
        chunks.append(audio)
        if sample_rate is not None:          # int16 from the GPU
            audio = np.ascontiguousarray(audio, np.int16).reshape(-1)
            if play:
                await loop.run_in_executor(None, _play, audio.astype(np.float32) / 32767.0, out_rate)
            yield audio.tobytes()
            continue
        if play:
            await loop.run_in_executor(None, _play, audio)
        yield A.to_pcm16(audio)
    if save_path and chunks:
        if sample_rate is not None:
            _write_pcm16_wav(os.fspath(save_path), b"".join(np.ascontiguousarray(c, np.int16).tobytes()
                                                            for c in chunks), out_rate)
        else:
            A.write_wav(os.fspath(save_path), np.concatenate(chunks), SAMPLE_RATE)


def wait_for_playback_done() -> None:
    """Playback is synchronous here (see `play`)."""


def stop() -> None:
    """TTSPlayer.stop (Core/TTSPlayer.py:208-222): the running sentence's decode is abandoned
    (GENIE.stop_event -> the engines' stop word) and the session ends: tts returns what was
    synthesized before the stop without saving, a tts_async iterator ends.  The next
    tts / tts_async call starts a new session."""
    _session_stop.set()
    tts_client.stop_event.set()
