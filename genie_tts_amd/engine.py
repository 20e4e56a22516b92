"""ctypes binding of libgenie_engine.so (C ABI: include/genie_engine.h).

PyTorch is plumbing here: device buffers are torch tensors whose data_ptr()
is handed to the engine, and calls run on torch's current HIP stream.  There
is no CPU fallback: if the library is missing or fails to load, every entry
point raises.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
import weakref
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import weights as W

# GENIE_ENGINE_LIB: an alternative build of the same library (A/B timing of a kernel variant)
_LIB_PATH = os.environ.get("GENIE_ENGINE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                                "libgenie_engine.so")
_lib = None

GSV_F32, GSV_F16 = 0, 1
GSV_V2, GSV_V2PP = 0, 1
MAX_BATCH = 64           # gsv_reserve: sequences decoded together


GSV_E_STOPPED = -6       # a generate abandoned by gsv_request_stop


class EngineError(RuntimeError):
    pass


class EngineStopped(EngineError):
    """A T2S generate was abandoned by a stop request (gsv_request_stop); the reference's
    loop returns None for the sentence then (Inference.py:96-97)."""


# Every live engine, so one stop request reaches them all, and the current request state for
# new engines.  The scope is the process, as in the reference: GENIE.stop_event belongs to the
# module-level tts_client (Core/Inference.py:13-14, 112) that every character shares, so a
# stop() ends the synthesis of every character.  _engines_lock orders registration against
# a stop request arriving from another thread.
_engines: "weakref.WeakSet" = weakref.WeakSet()
_engines_lock = threading.Lock()
_stop_on = False


def request_stop_all(on: bool) -> None:
    """Set (or clear) the stop word of every engine of this process (gsv_request_stop).
    Writes one host word per engine: safe from any thread while a generate runs."""
    global _stop_on
    with _engines_lock:
        _stop_on = bool(on)
        live = list(_engines)
        for e in live:
            if getattr(e, "h", None):
                lib().gsv_request_stop(e.h, int(on))


class Utt(ctypes.Structure):
    _fields_ = [
        ("ref_seq", ctypes.c_void_p), ("n_ref", ctypes.c_int32),
        ("text_seq", ctypes.c_void_p), ("n_text", ctypes.c_int32),
        ("ref_bert", ctypes.c_void_p), ("text_bert", ctypes.c_void_p),
        ("ssl", ctypes.c_void_p), ("n_ssl", ctypes.c_int32),
        ("force_steps", ctypes.c_int32),
    ]


class VitsItem(ctypes.Structure):
    _fields_ = [
        ("text_seq", ctypes.c_void_p), ("n_text", ctypes.c_int32),
        ("sem", ctypes.c_void_p), ("n_sem", ctypes.c_int32),
        ("ref_audio", ctypes.c_void_p), ("n_audio", ctypes.c_int32),
        ("ge", ctypes.c_void_p), ("ge_adv", ctypes.c_void_p),
        ("eps", ctypes.c_void_p), ("noise_seed", ctypes.c_uint64), ("noise_mode", ctypes.c_int32),
        ("audio", ctypes.c_void_p),
        ("speed", ctypes.c_float),
        ("out_rate", ctypes.c_int32), ("out_format", ctypes.c_int32),
        ("out", ctypes.c_void_p),
    ]


class Loudness(ctypes.Structure):
    """gsv_loudness: the loudness spec beside a vocoder item (target 0: off for that item)."""
    _fields_ = [("target", ctypes.c_float), ("peak", ctypes.c_float), ("stats", ctypes.c_void_p)]


class Join(ctypes.Structure):
    """gsv_join: gsv_loudness's fields plus the trim threshold (dBFS, 0: off), the pause (seconds)
    and the device span record int32[4] {begin, end, n_speech, n_out} (0: not wanted)."""
    _fields_ = [("target", ctypes.c_float), ("peak", ctypes.c_float), ("stats", ctypes.c_void_p),
                ("trim", ctypes.c_float), ("pause", ctypes.c_float), ("span", ctypes.c_void_p)]


class VocoderCall(NamedTuple):
    """One vocoder call as its C entry takes it, and what it will have written (Engine._vocoder_call).
    Holding it keeps every device buffer of the call alive."""
    items: Any            # the VitsItem array (None: the output stage alone, Engine.audio_convert)
    specs: Any            # the Join array beside it, or None (NULL): no item has a target, a pause or a trim
    keep: list            # the input tensors the items point at
    outs: list            # the result tensor of each item (its `out`, else its 32 kHz audio)
    a32: list             # the 32 kHz float32 tensor of each item
    stats: list           # the loudness stats of each item (device float32 [4]; None: no target)
    spans: list           # the span record of each item (device int32 [4]; None: no trim), rows of ...
    span_all: Any         # ... this one tensor [trimming items, 4] (None: no item trims)

    def joined(self, outs: Sequence) -> list:
        """outs (the call's results, after its wait) cut to their joined lengths: for an item with
        `trim`, out[:n_out] of its span record -- all the records of the call in one device-to-host
        copy; every other item as it is (with `pause` alone the length is known on the host and
        nothing is read back)."""
        if self.span_all is None:
            return list(outs)
        n_out = iter(self.span_all.cpu()[:, 3].tolist())
        return [o if sp is None else o[:next(n_out)] for o, sp in zip(outs, self.spans)]


class Sampler(ctypes.Structure):
    _fields_ = [
        ("top_k", ctypes.c_int32), ("temperature", ctypes.c_float),
        ("repetition_penalty", ctypes.c_float), ("greedy", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("max_steps", ctypes.c_int32),
        ("force_steps", ctypes.c_int32),
        ("top_p", ctypes.c_float),
    ]


SAMPLING_FIELDS = ("top_k", "top_p", "temperature", "repetition_penalty", "seed")


def check_sampling(top_k=None, top_p=None, temperature=None, repetition_penalty=None, seed=None) -> dict:
    """The sampling controls of a request (None: not given), validated: top_k 1..64,
    0 < top_p <= 1, temperature > 0, repetition_penalty > 0, seed a 64-bit unsigned integer.
    ValueError otherwise.  Returns the given ones as Sampler field values."""
    out = {}
    if top_k is not None:
        if isinstance(top_k, bool) or int(top_k) != top_k or not 1 <= int(top_k) <= 64:
            raise ValueError(f"top_k must be an integer in [1, 64], got {top_k!r}")
        out["top_k"] = int(top_k)
    for name, v, hi in (("top_p", top_p, 1.0), ("temperature", temperature, math.inf),
                        ("repetition_penalty", repetition_penalty, math.inf)):
        if v is None:
            continue
        v = float(v)
        if not (0.0 < v <= hi) or not math.isfinite(v):
            raise ValueError(f"{name} must be in (0, 1], got {v!r}" if name == "top_p"
                             else f"{name} must be a finite number > 0, got {v!r}")
        out[name] = v
    if seed is not None:
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        out["seed"] = int(seed)
    return out


def override_sampler(base: Sampler, **fields) -> Sampler:
    """A copy of `base` with the given (validated) sampling fields replaced."""
    sp = Sampler.from_buffer_copy(base)
    for k, v in check_sampling(**fields).items():
        setattr(sp, k, v)
    return sp


def sampler_key(sp: Sampler) -> tuple:
    """Every field of a sampler (top_p 0 read as 1): equal keys sample alike."""
    return tuple(1.0 if (n == "top_p" and getattr(sp, n) == 0) else getattr(sp, n) for n, _ in Sampler._fields_)


def make_sampler(top_k: int = 15, temperature: float = 1.0, repetition_penalty: float = 1.35,
                 greedy: bool = True, seed: int = 1234, max_steps: int = 500,
                 force_steps: int = 0, top_p: float = 1.0) -> Sampler:
    """Defaults are the constants baked into the reference graphs
    (t2s_stage_decoder_fp32.onnx#1780-1790, Inference.py:95).  top_p: the nucleus cut of
    GPT-SoVITS (0 < top_p <= 1, ValueError otherwise; 1: off, as the graphs were exported);
    sampled decoding only (include/genie_engine.h)."""
    check_sampling(top_p=top_p)
    return Sampler(top_k, temperature, repetition_penalty, int(greedy), seed, max_steps, force_steps, float(top_p))


class GemmDesc(ctypes.Structure):
    """gsv_gemm_desc (include/genie_engine.h): one gemm_nt launch, flat."""
    _fields_ = [(n, ctypes.c_int32) for n in ("M", "N", "K", "w_kind", "mode", "dry")] + [
        ("a", ctypes.c_void_p), ("lda", ctypes.c_int64),
        ("w", ctypes.c_void_p), ("wl", ctypes.c_void_p), ("ldw", ctypes.c_int64),
        ("bias", ctypes.c_void_p),
        ("c", ctypes.c_void_p), ("ldc", ctypes.c_int64),
        ("res", ctypes.c_void_p), ("ldr", ctypes.c_int64),
        ("rowsq", ctypes.c_void_p), ("colsq", ctypes.c_void_p),
        ("kv_k", ctypes.c_void_p), ("kv_v", ctypes.c_void_p), ("kv_tmax", ctypes.c_int32), ("kv_pos0", ctypes.c_int32),
        ("kv_row_pos", ctypes.c_void_p), ("kv_seq_stride", ctypes.c_int64), ("kv_row_seq", ctypes.c_void_p),
        ("kv_row_skip", ctypes.c_void_p),
        ("ksplit", ctypes.c_int32), ("a_nslab", ctypes.c_int32), ("slab_stride", ctypes.c_int64),
        ("a_slab_stride", ctypes.c_int64),
        ("a_bias", ctypes.c_void_p), ("a_relu", ctypes.c_int32), ("cus", ctypes.c_int32),
        ("ah", ctypes.c_void_p), ("al", ctypes.c_void_p), ("ch", ctypes.c_void_p), ("cl", ctypes.c_void_p),
        ("small_ns", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RowsDesc(ctypes.Structure):
    """gsv_rows_desc (include/genie_engine.h): one row-kernel launch."""
    _fields_ = [(n, ctypes.c_int32) for n in ("op", "rows", "D", "nslab")] + [
        ("in_", ctypes.c_void_p), ("out", ctypes.c_void_p), ("ld", ctypes.c_int64), ("slab_stride", ctypes.c_int64),
        ("g", ctypes.c_void_p), ("b", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p),
        ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p),
        ("eps", ctypes.c_float), ("reserved", ctypes.c_int32)]


_I32, _I64, _F32, _VP = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class ConvDesc(ctypes.Structure):
    """gsv_conv_desc (include/genie_engine.h): one conv1d launch, the fields of ConvArgs, flat."""
    _fields_ = [(n, _I32) for n in ("Cin", "Tin", "Cout", "K", "dil", "pad", "n_t", "o_tstride", "o_toff", "o_len",
                                    "in_act", "mode", "split", "phases", "tile_force", "ws", "dry", "deferred")] + [
        ("in_slope", _F32), ("div", _F32),
        ("x", _VP), ("x_cs", _I64), ("x_ts", _I64),
        ("w", _VP), ("bias", _VP),
        ("out", _VP), ("o_cs", _I64), ("o_ts", _I64),
        ("res", _VP), ("r_cs", _I64), ("r_ts", _I64),
        ("vec", _VP), ("acc", _VP), ("out2", _VP), ("res2", _VP),
        ("w_phase_stride", _I64),
        ("part", _VP), ("part_cap", _I64),
        ("wh", _VP), ("wscale", _VP), ("ovf", _VP), ("wh_phase_stride", _I64), ("in_scale", _VP),
        ("seg", _VP), ("vec_sstride", _I64)] + [
        (n, _I64) for n in ("n_x", "n_w", "n_out", "n_res", "n_acc", "n_out2", "n_seg")]


class MrfDesc(ctypes.Structure):
    """gsv_mrf_desc: one mrf_pair launch."""
    _fields_ = [(n, _I32) for n in ("T", "C", "K", "dil", "mode", "Cout", "n_t", "o_len", "o_tstride", "o_toff")] + [
        ("div", _F32), ("reserved", _I32),
        ("r", _VP), ("w1", _VP), ("s1", _VP), ("b1", _VP), ("w2", _VP), ("s2", _VP), ("bias2", _VP),
        ("ovf", _VP), ("out", _VP), ("acc", _VP), ("seg", _VP)] + [
        (n, _I64) for n in ("o_cs", "o_ts", "r_cs", "r_ts", "n_r", "n_out", "n_acc", "n_seg")]


class MhaDesc(ctypes.Structure):
    """gsv_mha_desc: one mha launch."""
    _fields_ = [(n, _I32) for n in ("nq", "nk", "heads", "dk", "postdiv", "window")] + [
        ("scale", _F32), ("reserved", _I32),
        ("q", _VP), ("q_ts", _I64), ("q_cs", _I64),
        ("k", _VP), ("k_ts", _I64), ("k_cs", _I64),
        ("v", _VP), ("v_ts", _I64), ("v_cs", _I64),
        ("out", _VP), ("o_ts", _I64), ("o_cs", _I64),
        ("ek", _VP), ("ev", _VP), ("row_seg", _VP), ("row_seg_host", _VP)] + [
        (n, _I64) for n in ("n_q", "n_k", "n_v", "n_out")]


class VitsRowsDesc(ctypes.Structure):
    """gsv_vits_rows_desc: one row kernel of csrc/vits.hip."""
    _fields_ = [(n, _I32) for n in ("op", "C", "T", "nsplit", "nseg", "f")] + [
        ("n", _I64), ("vec_sstride", _I64), ("div", _F32), ("reserved", _I32)] + [
        (n, _VP) for n in ("x", "y", "z", "out", "g", "b", "bias", "vec", "seg", "off", "len")]


class AttnDesc(ctypes.Structure):
    """gsv_attn_desc: one launch of a T2S attention kernel."""
    _fields_ = [(n, _I32) for n in ("form", "rows", "tmax", "len_add", "ntiles", "nslab", "dry", "reserved")] + [
        ("scale", _F32), ("reserved2", _I32),
        ("q", _VP), ("ldq", _I64), ("k", _VP), ("v", _VP), ("seq_stride", _I64),
        ("row_len", _VP), ("row_len_host", _VP), ("row_seq", _VP), ("row_seq_host", _VP), ("row_skip", _VP),
        ("out", _VP), ("ldo", _I64), ("tiles", _VP), ("tiles_host", _VP),
        ("slabs", _VP), ("slab_stride", _I64), ("b_in", _VP)]


class AttnOutDesc(ctypes.Structure):
    """gsv_attn_out_desc: one attn_outproj launch."""
    _fields_ = [("B", _I32), ("tmax", _I32), ("scale", _F32), ("reserved", _I32),
                ("q", _VP), ("k", _VP), ("v", _VP), ("seq_stride", _I64),
                ("kvlen", _VP), ("kvlen_host", _VP), ("done", _VP),
                ("WoT", _VP), ("part", _VP), ("acc_out", _VP), ("acc_bstride", _I64)]


class GemvDesc(ctypes.Structure):
    """gsv_gemv_desc: one gemv_f16 launch."""
    _fields_ = [(n, _I32) for n in ("B", "N", "K", "mode", "n_part", "kv_tmax", "kv_pos0", "reserved")] + [
        ("src", _VP), ("lds", _I64),
        ("part", _VP), ("part_stride", _I64), ("part_bias", _VP), ("part_res", _VP),
        ("acc_in", _VP), ("acc_bstride", _I64),
        ("ln_g", _VP), ("ln_b", _VP), ("ln_out", _VP), ("W", _VP), ("bias", _VP),
        ("C", _VP), ("ldc", _I64), ("res", _VP), ("ldr", _I64),
        ("kv_k", _VP), ("kv_v", _VP), ("kv_seq_stride", _I64),
        ("kv_row_pos", _VP), ("kv_row_pos_host", _VP), ("kv_row_skip", _VP)]


class FfnDesc(ctypes.Structure):
    """gsv_ffn_desc: one ffn_fused launch."""
    _fields_ = [("B", _I32), ("nslices", _I32)] + [
        (n, _VP) for n in ("h", "bo", "attn_part", "acc_attn", "ln_g", "ln_b", "h1", "W1", "b1", "W2T", "part",
                           "acc_out")] + [("acc_bstride", _I64)]


class EmbedDesc(ctypes.Structure):
    """gsv_embed_desc: one launch of an embedding kernel."""
    _fields_ = [(n, _I32) for n in ("op", "n", "n_tok", "n_pe")] + [
        ("tok", _VP), ("tok_host", _VP), ("ldy", _I64), ("ny", _VP), ("ny_host", _VP),
        ("emb", _VP), ("alpha", _VP), ("pe", _VP), ("out", _VP), ("done", _VP), ("ssl", _VP)]


# gsv_debug_attn's forms (the names it takes; "auto" reports "rows" or "flash") and gsv_debug_embed's ops
ATTN_FORMS = ("auto", "rows", "flash", "rowlane", "mf32", "dec_slabs")
EMBED_OPS = {"decode_embed": 0, "audio_embed_prompts": 1, "ssl_im2col": 2}
ATTN_SCALE = math.sqrt(1.0 / math.sqrt(32.0))     # applied to q and to k (t2s_stage_decoder #91-94)

# ConvMode (csrc/vits.h) and the paths gsv_debug_conv reports (ConvPath)
CONV_MODES = {"store": 0, "relu": 1, "resid": 2, "vec": 3, "sub": 4, "tanh": 5, "acc_first": 6, "acc_add": 7,
              "acc_mean": 8, "resid_vec": 9, "split_resid": 10}
CONV_PATHS = ("none", "f32", "f32_splitk", "conv_h", "conv_ws")
VITS_ROW_OPS = {"ln_channels": 0, "ln_channels_slabs": 1, "wn_gate": 2, "wn_gate_slabs": 3, "mean3": 4, "seg_fill": 5}

# gsv_debug_gemm's modes (EpiMode, csrc/kernels.h) and the forms it reports (GemmForm)
EPI = {"store": 0, "relu": 1, "resid": 2, "qkv": 3, "vqdist": 4, "mish": 5, "slab": 6, "gelu": 7, "relu_split": 8}
GEMM_FORMS = ("generic_f32", "generic_f16", "x2", "small_m2", "small_m3", "small_m4", "large_m", "large_m_ps",
              "split_w")
ROW_OPS = {"layernorm_rows": 0, "layernorm_rows_slabs": 1, "layernorm_rows_d": 2, "layernorm_rows_d_slabs": 3,
           "sumsq_rows": 4, "argmin_dist_rows": 5}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise EngineError(f"{_LIB_PATH} missing: build it with `python -m genie_tts_amd.build`")
        L = ctypes.CDLL(_LIB_PATH)
        vp, i32, i64p = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)
        L.gsv_last_error.restype = ctypes.c_char_p
        L.gsv_version.restype = ctypes.c_char_p
        if b"no packed-fp32" not in L.gsv_version():
            # built without build.py's NO_PACKED_FP32: its packed-FP32 ops can return 0 in lanes
            # 48-63 beside MFMA-heavy waves
            raise EngineError(f"{_LIB_PATH} was built with packed-FP32 ops: rebuild with "
                              "`python -m genie_tts_amd.build`")
        L.gsv_engine_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.gsv_engine_destroy.argtypes = [vp]
        L.gsv_set_weight.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_int, i64p, ctypes.c_int]
        L.gsv_finalize_weights.argtypes = [vp]
        L.gsv_reserve.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        L.gsv_t2s_encode.argtypes = [vp, ctypes.POINTER(Utt), vp, vp, vp]
        L.gsv_t2s_generate.argtypes = [vp, ctypes.c_int, ctypes.POINTER(Utt), ctypes.POINTER(Sampler),
                                       vp, i32, vp, vp]
        L.gsv_t2s_prefill.argtypes = [vp, ctypes.c_int, vp, i32, vp, i32, ctypes.POINTER(Sampler),
                                      vp, vp, vp]
        L.gsv_t2s_decode_steps.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Sampler),
                                           vp, vp, vp, vp]
        L.gsv_t2s_read_kv.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                      ctypes.POINTER(ctypes.c_int32), vp]
        L.gsv_vits_decode.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, ctypes.c_float, vp, vp]
        L.gsv_vits_decode_batch.argtypes = [vp, i32, ctypes.POINTER(VitsItem), ctypes.c_float, vp]
        L.gsv_vits_decode_async.argtypes = [vp, ctypes.POINTER(VitsItem), ctypes.c_float, vp]
        L.gsv_vits_wait.argtypes = [vp, vp]
        L.gsv_vits_frames.argtypes = [i32, ctypes.c_float]
        L.gsv_vits_decode_item.argtypes = [vp, ctypes.POINTER(VitsItem), ctypes.c_float, vp]
        L.gsv_debug_interp_linear.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
        L.gsv_audio_samples.argtypes = [i32, i32]
        L.gsv_audio_convert.argtypes = [vp, vp, i32, i32, i32, vp, vp]
        L.gsv_vits_decode_batch_async.argtypes = [vp, i32, ctypes.POINTER(VitsItem), ctypes.c_float, vp]
        ldp = ctypes.POINTER(Loudness)
        L.gsv_loudness_coeffs.argtypes = [i32, ctypes.POINTER(ctypes.c_double)]
        L.gsv_vits_decode_item_norm.argtypes = [vp, ctypes.POINTER(VitsItem), ldp, ctypes.c_float, vp]
        L.gsv_vits_decode_batch_norm.argtypes = [vp, i32, ctypes.POINTER(VitsItem), ldp, ctypes.c_float, vp]
        L.gsv_vits_decode_batch_async_norm.argtypes = [vp, i32, ctypes.POINTER(VitsItem), ldp, ctypes.c_float, vp]
        L.gsv_vits_decode_async_norm.argtypes = [vp, ctypes.POINTER(VitsItem), ldp, ctypes.c_float, vp]
        L.gsv_audio_loudness.argtypes = [vp, vp, i32, vp, vp]
        L.gsv_audio_normalize.argtypes = [vp, vp, i32, ctypes.c_float, ctypes.c_float, i32, i32, vp, vp, vp]
        L.gsv_debug_loudness_hops.argtypes = [vp, vp, i32, vp, vp]
        jnp = ctypes.POINTER(Join)
        L.gsv_join_pause_samples.argtypes = [i32, ctypes.c_float]
        L.gsv_join_samples.argtypes = [i32, i32, ctypes.c_float]
        L.gsv_vits_decode_item_join.argtypes = [vp, ctypes.POINTER(VitsItem), jnp, ctypes.c_float, vp]
        L.gsv_vits_decode_batch_join.argtypes = [vp, i32, ctypes.POINTER(VitsItem), jnp, ctypes.c_float, vp]
        L.gsv_vits_decode_batch_async_join.argtypes = [vp, i32, ctypes.POINTER(VitsItem), jnp, ctypes.c_float, vp]
        L.gsv_vits_decode_async_join.argtypes = [vp, ctypes.POINTER(VitsItem), jnp, ctypes.c_float, vp]
        L.gsv_audio_join.argtypes = [vp, vp, i32, jnp, i32, i32, vp, vp]
        L.gsv_debug_join_frames.argtypes = [vp, vp, i32, vp, vp]
        L.gsv_vits_batch_wait.argtypes = [vp, vp]
        L.gsv_t2s_prefetch.argtypes = [vp, ctypes.POINTER(Utt), ctypes.POINTER(Sampler), vp]
        L.gsv_t2s_generate_start.argtypes = [vp, ctypes.POINTER(Utt), ctypes.POINTER(Sampler), vp]
        L.gsv_t2s_generate_finish.argtypes = [vp, vp, i32, vp, vp]
        L.gsv_prompt_encode.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.gsv_ref_encode.argtypes = [vp, vp, i32, vp, vp]
        L.gsv_ge_mix.argtypes = [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_float), vp, vp]
        L.gsv_ge_project.argtypes = [vp, vp, vp, vp]
        L.gsv_debug_copy.argtypes = [vp, ctypes.c_char_p, vp, ctypes.c_int64, vp]
        L.gsv_debug_conv1d.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_float, vp, ctypes.c_int64, vp]
        L.gsv_debug_conv1d_h.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, vp, vp]
        L.gsv_debug_ktrace.argtypes = [vp, vp, ctypes.c_int]
        L.gsv_debug_sample.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(Sampler), ctypes.c_int, vp, vp, vp]
        L.gsv_t2s_generate_each.argtypes = [vp, ctypes.c_int, ctypes.POINTER(Utt), ctypes.POINTER(Sampler),
                                            ctypes.POINTER(ctypes.c_int32), vp, i32, vp, vp]
        L.gsv_debug_sample_each.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(Sampler),
                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_int, vp, vp, vp]
        L.gsv_probe.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_float), vp]
        L.gsv_set_timing.argtypes = [vp, ctypes.c_int]
        L.gsv_get_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.gsv_get_kernel_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)]
        L.gsv_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
        L.gsv_debug_ptrace.argtypes = [vp, vp, ctypes.c_int]
        L.gsv_get_counter.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
        L.gsv_hubert_frames.argtypes = [ctypes.c_int32]
        L.gsv_hubert.argtypes = [vp, vp, ctypes.c_int32, vp, vp]
        L.gsv_sv_frames.argtypes = [ctypes.c_int32]
        L.gsv_sv.argtypes = [vp, vp, ctypes.c_int32, vp, vp]
        L.gsv_roberta.argtypes = [vp, vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, vp]
        L.gsv_roberta_batch.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp, vp, vp]
        L.gsv_f16_exact.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        L.gsv_request_stop.argtypes = [vp, ctypes.c_int32]
        L.gsv_debug_hbm_copy.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_float)]
        L.gsv_debug_gemm.argtypes = [ctypes.POINTER(GemmDesc), vp, ctypes.POINTER(ctypes.c_int32)]
        L.gsv_debug_rows.argtypes = [ctypes.POINTER(RowsDesc), vp]
        L.gsv_debug_conv.argtypes = [ctypes.POINTER(ConvDesc), vp, ctypes.POINTER(ctypes.c_int32)]
        L.gsv_debug_mrf_pair.argtypes = [ctypes.POINTER(MrfDesc), vp]
        L.gsv_debug_mha.argtypes = [ctypes.POINTER(MhaDesc), vp]
        L.gsv_debug_vits_rows.argtypes = [ctypes.POINTER(VitsRowsDesc), vp]
        L.gsv_debug_attn.argtypes = [ctypes.POINTER(AttnDesc), vp, ctypes.POINTER(ctypes.c_int32)]
        L.gsv_debug_attn_out.argtypes = [ctypes.POINTER(AttnOutDesc), vp]
        L.gsv_debug_gemv.argtypes = [ctypes.POINTER(GemvDesc), vp]
        L.gsv_debug_ffn.argtypes = [ctypes.POINTER(FfnDesc), vp]
        L.gsv_debug_embed.argtypes = [ctypes.POINTER(EmbedDesc), vp]
        _lib = L
    return _lib


EXPORTED = (
    "gsv_last_error", "gsv_version", "gsv_engine_create", "gsv_engine_destroy", "gsv_set_weight",
    "gsv_finalize_weights", "gsv_reserve", "gsv_t2s_encode", "gsv_t2s_generate", "gsv_t2s_prefill",
    "gsv_t2s_decode_steps", "gsv_t2s_read_kv", "gsv_vits_decode", "gsv_prompt_encode",
    "gsv_set_timing", "gsv_get_timing", "gsv_debug_copy", "gsv_debug_conv1d",
    "gsv_probe", "gsv_get_kernel_timing", "gsv_debug_sample", "gsv_debug_ktrace",
    "gsv_set_option", "gsv_debug_ptrace", "gsv_debug_conv1d_h", "gsv_vits_decode_batch",
    "gsv_get_counter", "gsv_hubert", "gsv_hubert_frames", "gsv_sv", "gsv_sv_frames", "gsv_roberta",
    "gsv_vits_decode_async",
    "gsv_vits_wait", "gsv_t2s_prefetch", "gsv_t2s_generate_start", "gsv_t2s_generate_finish",
    "gsv_vits_decode_batch_async", "gsv_vits_batch_wait", "gsv_ref_encode", "gsv_roberta_batch",
    "gsv_f16_exact", "gsv_request_stop", "gsv_debug_hbm_copy", "gsv_vits_frames", "gsv_vits_decode_item",
    "gsv_debug_interp_linear", "gsv_t2s_generate_each", "gsv_debug_sample_each",
    "gsv_audio_samples", "gsv_audio_convert", "gsv_debug_gemm", "gsv_debug_rows",
    "gsv_debug_conv", "gsv_debug_mrf_pair", "gsv_debug_mha", "gsv_debug_vits_rows",
    "gsv_debug_attn", "gsv_debug_attn_out", "gsv_debug_gemv", "gsv_debug_ffn", "gsv_debug_embed",
    "gsv_loudness_coeffs", "gsv_vits_decode_item_norm", "gsv_vits_decode_batch_norm",
    "gsv_vits_decode_batch_async_norm", "gsv_vits_decode_async_norm", "gsv_audio_loudness",
    "gsv_audio_normalize", "gsv_debug_loudness_hops", "gsv_ge_mix", "gsv_ge_project",
    "gsv_join_pause_samples", "gsv_join_samples", "gsv_vits_decode_item_join", "gsv_vits_decode_batch_join",
    "gsv_vits_decode_batch_async_join", "gsv_vits_decode_async_join", "gsv_audio_join", "gsv_debug_join_frames",
)


def hbm_copy_ms(src, dst, iters: int = 10) -> float:
    """Mean time of one float4 grid-stride device copy src -> dst (torch tensors, same byte
    size), the achievable-HBM probe of bench.py (gsv_debug_hbm_copy)."""
    import torch
    ms = ctypes.c_float(0.0)
    nbytes = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() == nbytes and src.is_cuda and dst.is_cuda
    st = torch.cuda.current_stream(src.device).cuda_stream
    _check(lib().gsv_debug_hbm_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes,
                                    iters, ctypes.c_void_p(st), ctypes.byref(ms)), "hbm copy probe")
    return float(ms.value)


def f16_exact(values) -> int:
    """gsv_f16_exact: -1 when every value is exactly an fp16 number (what the engine's
    fp16-only weight paths require), else the index of the first one that is not.
    A host-only check: needs the library, not a GPU."""
    import numpy as np
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    bad = ctypes.c_int64(0)
    rc = lib().gsv_f16_exact(v.ctypes.data_as(ctypes.c_void_p), v.size, ctypes.byref(bad))
    if rc < 0:
        _check(rc, "gsv_f16_exact")
    return int(bad.value)


def vits_frames(n_sem: int, speed: float = 1.0) -> int:
    """Frames T' the vocoder runs at for n_sem semantic tokens at speech rate `speed`
    (gsv_vits_frames, the one place the count is computed; the audio is 640 T' samples).
    ValueError for a speed outside [0.25, 4] or not finite; 0 and 1 mean no resample."""
    try:
        sp = float(speed)
    except (TypeError, ValueError):
        raise ValueError(f"speed must be a number, not {speed!r}") from None
    n = lib().gsv_vits_frames(int(n_sem), ctypes.c_float(sp))
    if n < 0:
        raise ValueError(f"speed must be finite and within 0.25 .. 4.0, not {speed!r}")
    return n


SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def audio_samples(n: int, sample_rate: int = 32000) -> int:
    """Samples of n 32 kHz samples at sample_rate (gsv_audio_samples, the one place the length
    is computed: ceil(n * up / down)).  ValueError for a rate outside SAMPLE_RATES."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or \
            int(sample_rate) not in SAMPLE_RATES:
        raise ValueError(f"sample_rate must be one of {SAMPLE_RATES}, not {sample_rate!r}")
    m = lib().gsv_audio_samples(int(n), int(sample_rate))
    if m < 0:
        raise ValueError(f"no output length for {n!r} samples at {sample_rate!r} Hz")
    return m


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().gsv_last_error().decode(errors="replace")
        if rc == GSV_E_STOPPED:
            raise EngineStopped(f"{what}: {msg}")
        raise EngineError(f"{what} failed ({rc}): {msg}")


def check_out_format(sample_rate=None, pcm16=False) -> dict:
    """The output-format keys of a vocoder call that were given, validated (ValueError for a
    rate outside SAMPLE_RATES): nothing when neither is, and the call is then today's."""
    out = {}
    if sample_rate is not None:
        audio_samples(0, sample_rate)
        out["sample_rate"] = int(sample_rate)
    if pcm16:
        out["pcm16"] = True
    return out


def check_loudness(loudness=None, peak=None) -> dict:
    """The loudness keys of a vocoder call, validated: `loudness` a target in LUFS within
    [-50, -5], `peak` a linear sample-peak ceiling in (0, 1] (None: -1 dBFS).  ValueError
    otherwise.  Nothing when loudness is None, and the call is then today's."""
    out = {}
    for name, v, lo, hi in (("loudness", loudness, -50.0, -5.0), ("peak", peak, 0.0, 1.0)):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not math.isfinite(float(v)) or not lo <= float(v) <= hi or (name == "peak" and float(v) == 0.0):
            raise ValueError(f"loudness must be a target in LUFS within [-50, -5], not {v!r}" if name == "loudness"
                             else f"peak must be a linear ceiling in (0, 1], not {v!r}")
        out[name] = float(v)
    return out if loudness is not None else {}


JOIN_FRAME = 320          # GSV_JOIN_FRAME: samples of a trim frame (10 ms at 32 kHz)
JOIN_GUARD = 640          # GSV_JOIN_GUARD: samples kept on either side of the active frames (20 ms)


def check_join(pause=None, trim=None) -> dict:
    """The join keys of a vocoder call, validated: `pause` seconds of silence behind the sentence
    within [0, 5] (None or 0: none), `trim` a threshold in dBFS within [-80, -20] (None: nothing
    is cut).  ValueError otherwise.  Nothing when neither is given, and the call is then today's."""
    out = {}
    for name, v, lo, hi in (("pause", pause, 0.0, 5.0), ("trim", trim, -80.0, -20.0)):
        if v is None:
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not math.isfinite(float(v)) or not lo <= float(v) <= hi:
            raise ValueError(f"pause must be seconds within [0, 5], not {v!r}" if name == "pause"
                             else f"trim must be a threshold in dBFS within [-80, -20], not {v!r}")
        if name == "trim" or float(v) != 0.0:
            out[name] = float(v)
    return out


def join_pause_samples(sample_rate: int = 32000, pause: float = 0.0) -> int:
    """Samples of `pause` seconds at sample_rate (gsv_join_pause_samples, the one place the count
    is computed: (int)((double)rate * (double)(float32)pause))."""
    audio_samples(0, sample_rate)
    n = lib().gsv_join_pause_samples(int(sample_rate), ctypes.c_float(float(pause)))
    if n < 0:
        raise ValueError(f"pause must be seconds within [0, 5], not {pause!r}")
    return n


def join_samples(n: int, sample_rate: int = 32000, pause: float = 0.0) -> int:
    """The most samples a joined item gives (gsv_join_samples): audio_samples(n, sample_rate)
    plus the pause's; what its output buffer must hold."""
    audio_samples(0, sample_rate)
    m = lib().gsv_join_samples(int(n), int(sample_rate), ctypes.c_float(float(pause)))
    if m < 0:
        raise ValueError(f"no output length for {n!r} samples at {sample_rate!r} Hz with a pause of {pause!r}")
    return m


VOCODER_OPTIONS = ("speed", "sample_rate", "pcm16", "loudness", "peak", "pause", "trim")


def vocoder_options(speed=None, sample_rate=None, pcm16=False, loudness=None, peak=None, pause=None,
                    trim=None) -> dict:
    """The options of one vocoder call, validated (ValueError, before any GPU work), as the
    keywords of Engine.vits_decode / the keys of a vocoder item.  Only what differs from the
    call without options is returned, so nothing given is that call, with no extra keyword.
    speed: the speech rate (GPT-SoVITS's `speed`), finite and within 0.25 .. 4; the vocoder
      runs at T' = vits_frames(G, speed) frames and the audio is 640 T' samples, its pitch
      unchanged.  No key for None or 1.
    sample_rate / pcm16: the output stage behind the vocoder, on the GPU (Engine.audio_convert):
      the audio at one of SAMPLE_RATES, audio_samples(640 T', sample_rate) samples, and / or as
      saturated int16.  Neither: float32 at 32 kHz.
    loudness / peak: the audio measured by ITU-R BS.1770-4 and brought to `loudness` LUFS
      (within [-50, -5]; e.g. -16 for speech, EBU R 128's -23) on the GPU, in front of the
      conversion, the gain limited so that the 32 kHz sample peak stays under `peak` (linear,
      (0, 1]; None: -1 dBFS).  With loudness alone the audio is float32 at 32 kHz, normalised.
      A `peak` without a `loudness` is validated and dropped.
    pause / trim: the sentence join, on the GPU in the same stage.  `trim` (dBFS, -80 .. -20) cuts
      the leading and trailing audio quieter than it, down to a guard of 20 ms; `pause` (seconds,
      0 .. 5; GPT-SoVITS's `fragment_interval`) appends silence.  The result then has as many
      samples as the span record says (Engine.vits_joined).  No key for a pause of None or 0."""
    out = {}
    if speed is not None:
        vits_frames(0, speed)
        if float(speed) != 1.0:
            out["speed"] = float(speed)
    out.update(check_out_format(sample_rate, pcm16))
    out.update(check_loudness(loudness, peak))
    out.update(check_join(pause, trim))
    return out


def vocoder_options_each(n: int, speed=1.0, sample_rate=None, pcm16=False, loudness=None, peak=None, pause=None,
                         trim=None) -> List[dict]:
    """vocoder_options of n items, each option one value for all of them or one per item."""
    cols = [[v] * n if v is None or np.ndim(v) == 0 else list(v)
            for v in (speed, sample_rate, pcm16, loudness, peak, pause, trim)]
    for what, group in (("speed", cols[:1]), ("sample_rate / pcm16", cols[1:3]), ("loudness / peak", cols[3:5]),
                        ("pause / trim", cols[5:])):
        if any(len(c) != n for c in group):
            raise ValueError(f"{what}: one value, or one per item")
    return [vocoder_options(*row) for row in zip(*cols)]


MIX_MAX = 16             # GSV_MIX_MAX: clips of one fused reference


def mix_weights(n: int, weights=None) -> np.ndarray:
    """The float32 [n] weights of a timbre fusion over n reference clips, primary first
    (gsv_ge_mix multiplies exactly these): None is equal weights, GPT-SoVITS's plain mean; given
    weights are normalised to sum 1 in float64 and rounded once to float32.  The one place they
    are checked: ValueError for n outside 1 .. MIX_MAX, a wrong length, a bool, a non-finite or
    negative entry, or a zero sum.  Needs no GPU."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MIX_MAX:
        raise ValueError(f"a fused reference has 1 .. {MIX_MAX} clips, not {n!r}")
    n = int(n)
    if weights is None:
        return np.full(n, 1.0 / n, np.float64).astype(np.float32)
    if np.ndim(weights) != 1 or len(weights) != n:
        raise ValueError(f"weights: one per clip, primary first ({n}), not {weights!r}")
    for i, v in enumerate(weights):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"weights[{i}] must be a number, not {v!r}")
        if not math.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError(f"weights[{i}] must be finite and >= 0, not {v!r}")
    w = np.array([float(v) for v in weights], np.float64)
    total = float(w.sum())
    if not total > 0.0:
        raise ValueError("weights: at least one must be above 0")
    return (w / total).astype(np.float32)


def loudness_coeffs(rate: int):
    """gsv_loudness_coeffs: the K-weighting biquads at `rate` as float64 [10] (shelf b0 b1 b2 a1
    a2, high-pass b0 b1 b2 a1 a2).  Host only: needs the library, not a GPU."""
    out = (ctypes.c_double * 10)()
    _check(lib().gsv_loudness_coeffs(int(rate), out), "gsv_loudness_coeffs")
    return np.array(out[:], np.float64)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise EngineError("no HIP device visible: the MI355X engine has no CPU fallback")
    return torch


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def debug_conv1d(x, w, bias=None, dil=1, pad=0, in_act=False, slope=0.1, splitk_ws=None):
    """Run the engine's conv1d kernel once (tests): x [Cin,T], w [Cout,Cin,K] cuda fp32.
    splitk_ws (cuda fp32 tensor) enables the split-K path for small grids."""
    torch = _torch()
    cin, tin = x.shape
    cout, _, k = w.shape
    tout = tin + 2 * pad - dil * (k - 1)
    out = torch.empty((cout, tout), dtype=torch.float32, device=x.device)
    _check(lib().gsv_debug_conv1d(_ptr(x), cin, tin, _ptr(w), cout, k, dil, pad, _ptr(bias), _ptr(out),
                                  tout, int(in_act), ctypes.c_float(slope), _ptr(splitk_ws),
                                  0 if splitk_ws is None else splitk_ws.numel(), _stream()), "gsv_debug_conv1d")
    return out


def debug_conv1d_h(x, v, scale, bias=None, dil=1, pad=0, in_act=False, slope=0.1):
    """Run the f16-split MFMA conv once (tests): x [Cin,T] cuda fp32, v [Cout,Cin,K] fp16-valued,
    scale [Cout] (weight = v * scale).  Returns (out, overflow flag)."""
    torch = _torch()
    cin, tin = x.shape
    cout, _, k = v.shape
    tout = tin + 2 * pad - dil * (k - 1)
    wh = v.to(torch.float16).permute(0, 2, 1).contiguous().to(x.device)     # [Cout][K][Cin]
    sc = scale.to(torch.float32).contiguous().to(x.device)
    out = torch.empty((cout, tout), dtype=torch.float32, device=x.device)
    ovf = torch.zeros(1, dtype=torch.int32, device=x.device)
    _check(lib().gsv_debug_conv1d_h(_ptr(x), cin, tin, _ptr(wh), _ptr(sc), cout, k, dil, pad, _ptr(bias), _ptr(out),
                                    tout, int(in_act), ctypes.c_float(slope), _ptr(ovf), _stream()),
           "gsv_debug_conv1d_h")
    return out, int(ovf.item())


def gemm_desc(M, N, K, *, w_kind=1, mode="store", dry=False, **f) -> GemmDesc:
    """A GemmDesc from sizes and fields; a field is an int, None, or anything with data_ptr()."""
    d = GemmDesc()
    d.M, d.N, d.K, d.w_kind, d.mode, d.dry = M, N, K, w_kind, EPI[mode] if isinstance(mode, str) else mode, int(dry)
    for k, v in f.items():
        if not hasattr(d, k):
            raise TypeError(f"gsv_gemm_desc has no field {k}")
        setattr(d, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return d


def debug_gemm_form(M, N, K, **f) -> str:
    """The kernel gemm_nt would launch (a name of GEMM_FORMS), from the hook's dry path: no HIP
    call, so the pointers may be any aligned non-zero integers.  EngineError for a refused set."""
    form = ctypes.c_int32(-1)
    _check(lib().gsv_debug_gemm(ctypes.byref(gemm_desc(M, N, K, dry=True, **f)), None, ctypes.byref(form)),
           "gsv_debug_gemm")
    return GEMM_FORMS[form.value]


def debug_gemm(M, N, K, **f) -> str:
    """Run gemm_nt once on cuda tensors (tests; the fields of gsv_gemm_desc by name: a, lda, w, wl,
    ldw, bias, c, ldc, mode, ...) on the current stream; returns the form that ran."""
    form = ctypes.c_int32(-1)
    _check(lib().gsv_debug_gemm(ctypes.byref(gemm_desc(M, N, K, **f)), _stream(), ctypes.byref(form)),
           "gsv_debug_gemm")
    return GEMM_FORMS[form.value]


def debug_rows(op: str, rows: int, D: int, inp, out, **f):
    """Run one row kernel (a name of ROW_OPS) on cuda tensors; fields of gsv_rows_desc by name."""
    d = RowsDesc()
    d.op, d.rows, d.D = ROW_OPS[op], rows, D
    d.in_, d.out = inp.data_ptr(), out.data_ptr()
    for k, v in f.items():
        if not hasattr(d, k):
            raise TypeError(f"gsv_rows_desc has no field {k}")
        setattr(d, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    _check(lib().gsv_debug_rows(ctypes.byref(d), _stream() if rows > 0 else None), "gsv_debug_rows")


def _fill(d, fields, sizes=()):
    """Set a desc's fields by name: an int / float, None, or a tensor (its data_ptr; for a name of
    `sizes`, n_<name> = its element count unless given)."""
    for k, v in fields.items():
        if not hasattr(d, k):
            raise TypeError(f"{type(d).__name__} has no field {k}")
        if hasattr(v, "data_ptr"):
            if k in sizes and "n_" + sizes[k] not in fields:
                setattr(d, "n_" + sizes[k], v.numel())
            v = v.data_ptr()
        setattr(d, k, v)
    return d


_CONV_SIZES = {"x": "x", "w": "w", "wh": "w", "out": "out", "res": "res", "acc": "acc", "out2": "out2", "seg": "seg"}


def conv_desc(*, mode="store", **f) -> ConvDesc:
    """A ConvDesc from fields by name.  Defaults: dil 1, one phase, o_tstride 1, unit time strides,
    in_slope 0.1, div 1; n_<buffer> from the tensors given; part_cap from part."""
    d = ConvDesc()
    d.dil = d.o_tstride = d.x_ts = d.o_ts = d.r_ts = d.phases = 1
    d.in_slope, d.div = 0.1, 1.0
    d.mode = CONV_MODES[mode] if isinstance(mode, str) else mode
    if hasattr(f.get("part"), "numel") and "part_cap" not in f:
        d.part_cap = f["part"].numel()
    return _fill(d, f, _CONV_SIZES)


def debug_conv(desc=None, stream=True, **f) -> dict:
    """gsv_debug_conv on a ConvDesc (or the fields of conv_desc): one conv1d launch on the current
    stream (stream = None: none is passed, for the dry path and the rejections, which make no HIP
    call).  Returns the form: path (a name of CONV_PATHS) and nsplit, v4 (f32) or chunk, tile
    (f16), and the slabs a deferred launch left."""
    d = desc if desc is not None else conv_desc(**f)
    form = (ctypes.c_int32 * 4)()
    _check(lib().gsv_debug_conv(ctypes.byref(d), _stream() if stream and not d.dry else None, form), "gsv_debug_conv")
    path = CONV_PATHS[form[0]]
    if path in ("conv_h", "conv_ws"):
        return {"path": path, "chunk": form[1], "tile": form[2], "slabs": form[3]}
    return {"path": path, "nsplit": form[1], "v4": bool(form[2]), "slabs": form[3]}


def debug_mrf_pair(stream=True, *, mode="resid", **f):
    """gsv_debug_mrf_pair: one fused ResBlock step; T, C, K, dil and the tensors r, w1, s1, b1, w2,
    s2, bias2, ovf, out / acc (seg) by name.  The epilogue's geometry defaults to mrf_pair's own."""
    d = MrfDesc()
    T, C = f["T"], f["C"]
    d.Cout, d.n_t, d.o_len, d.o_tstride, d.o_toff = C, T, T, 1, 0
    d.o_cs, d.o_ts, d.r_cs, d.r_ts, d.div = T, 1, T, 1, 1.0
    d.mode = CONV_MODES[mode] if isinstance(mode, str) else mode
    _fill(d, f, {"r": "r", "out": "out", "acc": "acc", "seg": "seg"})
    _check(lib().gsv_debug_mrf_pair(ctypes.byref(d), _stream() if stream else None), "gsv_debug_mrf_pair")


def debug_mha(stream=True, **f):
    """gsv_debug_mha: one attention launch; the fields of gsv_mha_desc by name (row_seg_host: an
    int32 numpy array, kept alive by the caller's reference for the call)."""
    d = MhaDesc()
    d.scale = 1.0
    host = f.pop("row_seg_host", None)
    if host is not None:
        host = np.ascontiguousarray(host, np.int32)
        d.row_seg_host = host.ctypes.data
    _fill(d, f, {"q": "q", "k": "k", "v": "v", "out": "out"})
    _check(lib().gsv_debug_mha(ctypes.byref(d), _stream() if stream else None), "gsv_debug_mha")


def debug_vits_rows(op: str, stream=True, **f):
    """gsv_debug_vits_rows: one row kernel of csrc/vits.hip (a name of VITS_ROW_OPS)."""
    d = VitsRowsDesc()
    d.op, d.div = VITS_ROW_OPS[op] if isinstance(op, str) else op, 1.0
    _fill(d, f)
    _check(lib().gsv_debug_vits_rows(ctypes.byref(d), _stream() if stream else None), "gsv_debug_vits_rows")


def _fill_host(d, f, names):
    """_fill, with the host copies `names` (numpy arrays of the dtype given) kept alive by the list returned."""
    keep = []
    for k, dt in names.items():
        h = f.pop(k, None)
        if h is not None:
            h = np.ascontiguousarray(h, dt)
            keep.append(h)
            setattr(d, k, h.ctypes.data)
    _fill(d, f)
    return keep


def attn_desc(form="auto", dry=False, **f) -> AttnDesc:
    """An AttnDesc from fields by name (form: a name of ATTN_FORMS); scale defaults to ATTN_SCALE,
    ldq / ldo to 512.  row_len_host, row_seq_host, tiles_host: int32 arrays, referenced by d._keep."""
    d = AttnDesc()
    d.form, d.dry, d.scale, d.ldq, d.ldo = ATTN_FORMS.index(form) if isinstance(form, str) else form, int(dry), \
        ATTN_SCALE, 512, 512
    d._keep = _fill_host(d, f, {"row_len_host": np.int32, "row_seq_host": np.int32, "tiles_host": np.int32})
    return d


def debug_attn(form="auto", stream=True, **f) -> str:
    """gsv_debug_attn: one launch of a T2S attention kernel on the current stream (stream = None
    with dry=True: no HIP call); returns the form that ran (a name of ATTN_FORMS)."""
    d = attn_desc(form, **f)
    ran = ctypes.c_int32(-1)
    _check(lib().gsv_debug_attn(ctypes.byref(d), _stream() if stream and not d.dry else None, ctypes.byref(ran)),
           "gsv_debug_attn")
    return ATTN_FORMS[ran.value]


def debug_attn_out(**f):
    """gsv_debug_attn_out: one attn_outproj launch; the fields of gsv_attn_out_desc by name."""
    d = AttnOutDesc()
    d.scale = ATTN_SCALE
    keep = _fill_host(d, f, {"kvlen_host": np.int32})
    _check(lib().gsv_debug_attn_out(ctypes.byref(d), _stream()), "gsv_debug_attn_out")
    del keep


def debug_gemv(mode="store", **f):
    """gsv_debug_gemv: one gemv_f16 launch; the fields of gsv_gemv_desc by name (mode: a name of EPI)."""
    d = GemvDesc()
    d.mode = EPI[mode] if isinstance(mode, str) else mode
    keep = _fill_host(d, f, {"kv_row_pos_host": np.int32})
    _check(lib().gsv_debug_gemv(ctypes.byref(d), _stream()), "gsv_debug_gemv")
    del keep


def debug_ffn(**f):
    """gsv_debug_ffn: one ffn_fused launch; the fields of gsv_ffn_desc by name."""
    _check(lib().gsv_debug_ffn(ctypes.byref(_fill(FfnDesc(), f)), _stream()), "gsv_debug_ffn")


def debug_embed(op: str, **f):
    """gsv_debug_embed: one launch of an embedding kernel (a name of EMBED_OPS)."""
    d = EmbedDesc()
    d.op = EMBED_OPS[op] if isinstance(op, str) else op
    keep = _fill_host(d, f, {"tok_host": np.int64, "ny_host": np.int32})
    _check(lib().gsv_debug_embed(ctypes.byref(d), _stream()), "gsv_debug_embed")
    del keep


def debug_sample(logits, seen, sampler: "Sampler", step: int):
    """Run the decode sampler kernel (tests): logits [B,1025] cuda f32, seen [B,33] cuda int32 bitmaps."""
    torch = _torch()
    B = logits.shape[0]
    tok = torch.empty((B,), dtype=torch.int64, device=logits.device)
    stop = torch.empty((B,), dtype=torch.uint8, device=logits.device)
    _check(lib().gsv_debug_sample(_ptr(logits), _ptr(seen), B, ctypes.byref(sampler), step, _ptr(tok), _ptr(stop),
                                  _stream()), "gsv_debug_sample")
    return tok, stop


def _each_args(n: int, samplers, streams):
    """The (samplers, streams) arrays of a per-sequence call over n sequences: one Sampler per
    sequence; streams None (the slot numbering) or n integers >= 0.  ValueError otherwise."""
    samplers = list(samplers)
    if len(samplers) != n:
        raise ValueError(f"samplers: {len(samplers)} entries for {n} sequences")
    if not all(isinstance(sp, Sampler) for sp in samplers):
        raise ValueError("samplers: every entry must be a Sampler")
    sarr = (Sampler * n)(*samplers)
    if streams is None:
        return sarr, None
    streams = list(streams)
    if len(streams) != n:
        raise ValueError(f"streams: {len(streams)} entries for {n} sequences")
    for i, v in enumerate(streams):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 1 << 31:
            raise ValueError(f"streams[{i}] must be an integer in [0, 2^31), got {v!r}")
    return sarr, (ctypes.c_int32 * n)(*[int(v) for v in streams])


def debug_sample_each(logits, seen, samplers, step: int, streams=None):
    """debug_sample with one Sampler (and Philox stream; None: the row index) per row
    (gsv_debug_sample_each)."""
    torch = _torch()
    B = logits.shape[0]
    sarr, starr = _each_args(B, samplers, streams)
    tok = torch.empty((B,), dtype=torch.int64, device=logits.device)
    stop = torch.empty((B,), dtype=torch.uint8, device=logits.device)
    _check(lib().gsv_debug_sample_each(_ptr(logits), _ptr(seen), B, sarr, starr, step, _ptr(tok), _ptr(stop),
                                       _stream()), "gsv_debug_sample_each")
    return tok, stop


class Engine:
    """One engine per GPU process, holding one character's weights."""

    def __init__(self, weights: Dict[str, Dict[str, np.ndarray]], version: str = "v2",
                 device: int = 0, pe_div_term: Optional[np.ndarray] = None):
        torch = _torch()
        self.torch = torch
        self.device = device
        self.version = version
        torch.cuda.set_device(device)
        h = ctypes.c_void_p()
        _check(lib().gsv_engine_create(device, GSV_V2 if version == "v2" else GSV_V2PP,
                                       ctypes.byref(h)), "gsv_engine_create")
        self.h = h
        for group in weights.values():
            for name, arr in group.items():
                self._set(name, arr)
        if pe_div_term is not None:
            self._set("pe.div_term", np.asarray(pe_div_term, np.float32))
        _check(lib().gsv_finalize_weights(self.h), "gsv_finalize_weights")
        self.dev = torch.device("cuda", device)
        with _engines_lock:
            _engines.add(self)
            if _stop_on:
                lib().gsv_request_stop(self.h, 1)

    def request_stop(self, on: bool = True):
        """gsv_request_stop: while set, T2S generates raise EngineStopped (a running decode
        leaves within two loop steps).  Callable from another thread."""
        _check(lib().gsv_request_stop(self.h, int(on)), "gsv_request_stop")

    def _set(self, name: str, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        if a.dtype == np.float16:
            dt = GSV_F16
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            dt = GSV_F32
        dims = (ctypes.c_int64 * max(1, a.ndim))(*a.shape)
        _check(lib().gsv_set_weight(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), dt,
                                    dims, a.ndim), f"gsv_set_weight({name})")

    def close(self):
        if getattr(self, "h", None):
            lib().gsv_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- helpers
    def _dev(self, x, dtype):
        t = self.torch
        if x is None:
            return None
        if isinstance(x, t.Tensor):
            return x.to(device=self.dev, dtype=dtype).contiguous()
        return t.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=self.dev).contiguous()

    def make_utt(self, ref_seq, text_seq, ref_bert, text_bert, ssl, force_steps: int = 0):
        t = self.torch
        flat = lambda a: a.reshape(-1) if isinstance(a, t.Tensor) else np.asarray(a).reshape(-1)
        keep = [self._dev(flat(ref_seq), t.int64),
                self._dev(flat(text_seq), t.int64),
                None if ref_bert is None else self._dev(ref_bert, t.float32),
                None if text_bert is None else self._dev(text_bert, t.float32),
                self._dev(ssl, t.float32).reshape(768, -1)]
        u = Utt(keep[0].data_ptr(), keep[0].numel(), keep[1].data_ptr(), keep[1].numel(),
                0 if keep[2] is None else keep[2].data_ptr(),
                0 if keep[3] is None else keep[3].data_ptr(),
                keep[4].data_ptr(), keep[4].shape[1], int(force_steps))
        return u, keep

    def reserve(self, batch: int, tokens: int):
        _check(lib().gsv_reserve(self.h, batch, tokens), "gsv_reserve")

    # -------------------------------------------------------------- T2S
    def t2s_encode(self, ref_seq, text_seq, ref_bert, text_bert, ssl):
        t = self.torch
        u, keep = self.make_utt(ref_seq, text_seq, ref_bert, text_bert, ssl)
        L = u.n_ref + u.n_text
        x = t.empty((L, 512), dtype=t.float32, device=self.dev)
        prompts = t.empty((u.n_ssl // 2,), dtype=t.int64, device=self.dev)
        _check(lib().gsv_t2s_encode(self.h, ctypes.byref(u), _ptr(x), _ptr(prompts), _stream()),
               "gsv_t2s_encode")
        return x, prompts

    def t2s_generate(self, utts: Sequence[Tuple], sampler: Optional[Sampler] = None,
                     out_stride: int = 1024, *, samplers: Optional[Sequence[Sampler]] = None,
                     streams: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        """utts: sequence of (ref_seq, text_seq, ref_bert, text_bert, ssl[, force_steps]);
        force_steps > 0 runs that utterance for exactly that many loop steps (EOS ignored).

        samplers: one Sampler per utterance instead of `sampler` (gsv_t2s_generate_each: one
        launch, every sequence sampling with its own controls; max_steps equal in all).
        streams: with samplers, the Philox stream word per utterance (None: its slot, as
        without samplers; 0: the noise of a batch-1 generate).  ValueError for a wrong length,
        a bad stream or both sampler arguments."""
        if samplers is None:
            if streams is not None:
                raise ValueError("streams needs samplers")
        else:
            if sampler is not None:
                raise ValueError("sampler and samplers are exclusive")
            sarr, starr = _each_args(len(utts), samplers, streams)   # (validates the whole lists)
        if len(utts) > MAX_BATCH:   # the engine decodes up to 64 sequences together
            out = []
            for i in range(0, len(utts), MAX_BATCH):
                j = i + MAX_BATCH
                if samplers is None:
                    out += self.t2s_generate(utts[i:j], sampler, out_stride)
                else:
                    out += self.t2s_generate(utts[i:j], None, out_stride, samplers=list(samplers)[i:j],
                                             streams=None if streams is None else list(streams)[i:j])
            return out
        arr = (Utt * len(utts))()
        keep = []
        pf = getattr(self, "_pf", [])
        hit = next((j for j, p in enumerate(pf) if len(utts) == 1 and p[0] is utts[0]), None)
        if samplers is not None:
            hit = None   # (the engine takes no prefetched utterance on this path)
        # consumed entries go; on a single-utterance miss the engine keeps a queued
        # prefetch (the latest), whose buffers must stay alive; a batch drops all
        self._pf = pf[hit + 1:] if hit is not None else pf[-1:] if len(utts) == 1 else []
        for i, u in enumerate(utts):
            if hit is not None:
                arr[i], k = pf[hit][1], pf[hit][2]   # the prefetched utterance: the same device buffers
            else:
                arr[i], k = self.make_utt(*u)
            keep.append(k)
        out = np.zeros((len(utts), out_stride), dtype=np.int64)
        lens = np.zeros(len(utts), dtype=np.int32)
        if samplers is not None:
            _check(lib().gsv_t2s_generate_each(self.h, len(utts), arr, sarr, starr,
                                               out.ctypes.data_as(ctypes.c_void_p), out_stride,
                                               lens.ctypes.data_as(ctypes.c_void_p), _stream()),
                   "gsv_t2s_generate_each")
            return [out[i, :lens[i]].copy() for i in range(len(utts))]
        sp = sampler or make_sampler()
        _check(lib().gsv_t2s_generate(self.h, len(utts), arr, ctypes.byref(sp),
                                      out.ctypes.data_as(ctypes.c_void_p), out_stride,
                                      lens.ctypes.data_as(ctypes.c_void_p), _stream()),
               "gsv_t2s_generate")
        return [out[i, :lens[i]].copy() for i in range(len(utts))]

    def t2s_prefetch(self, utt: Tuple, sampler: Optional[Sampler] = None):
        """Encode + prefill `utt` (a t2s_generate tuple) ahead on the vocoder CUs while the
        current decode runs (gsv_t2s_prefetch); the next t2s_generate([utt], sampler)
        with this same tuple object decodes from it."""
        u, keep = self.make_utt(*utt)
        sp = sampler or make_sampler()
        _check(lib().gsv_t2s_prefetch(self.h, ctypes.byref(u), ctypes.byref(sp), _stream()), "gsv_t2s_prefetch")
        # the engine holds a launched prefetch (for the next generate) and a queued one
        self._pf = (getattr(self, "_pf", []) + [(utt, u, keep)])[-2:]

    def t2s_generate_start(self, utt: Tuple, sampler: Optional[Sampler] = None):
        """Queue the T2S of one utterance (gsv_t2s_generate_start) and return at once;
        up to two in flight: on two decode lanes side by side where the CU split leaves >= 192
        decode CUs (option decode_lanes), else the next decode queued behind the running one.
        t2s_generate_finish() returns the oldest one's tokens."""
        pf = getattr(self, "_pf", [])
        hit = next((j for j, p in enumerate(pf) if p[0] is utt), None)
        if hit is not None:
            u, keep = pf[hit][1], pf[hit][2]
            self._pf = pf[hit + 1:]
        else:
            u, keep = self.make_utt(*utt)
            self._pf = pf[-1:]
        sp = sampler or make_sampler()
        _check(lib().gsv_t2s_generate_start(self.h, ctypes.byref(u), ctypes.byref(sp), _stream()),
               "gsv_t2s_generate_start")
        if not hasattr(self, "_gq"):
            self._gq = []
        self._gq.append((u, keep))

    def t2s_generate_finish(self, out_stride: int = 1024) -> np.ndarray:
        """Tokens of the oldest started generate (trimmed, EOS-filtered)."""
        out = np.zeros((out_stride,), dtype=np.int64)
        n = np.zeros(1, dtype=np.int32)
        try:
            _check(lib().gsv_t2s_generate_finish(self.h, out.ctypes.data_as(ctypes.c_void_p), out_stride,
                                                 n.ctypes.data_as(ctypes.c_void_p), _stream()),
                   "gsv_t2s_generate_finish")
        finally:
            if getattr(self, "_gq", None):
                self._gq.pop(0)
        return out[:n[0]].copy()

    def t2s_prefill(self, x, prompts, sampler: Optional[Sampler] = None, seq: int = 0):
        t = self.torch
        x = self._dev(x, t.float32).reshape(-1, 512)
        prompts = self._dev(np.asarray(prompts).reshape(-1) if not isinstance(prompts, t.Tensor)
                            else prompts.reshape(-1), t.int64)
        L, P = x.shape[0], prompts.numel()
        self.reserve(max(1, seq + 1), L + P + 520)
        y = t.empty((P + 1,), dtype=t.int64, device=self.dev)
        logits = t.empty((1025,), dtype=t.float32, device=self.dev)
        sp = sampler or make_sampler()
        _check(lib().gsv_t2s_prefill(self.h, seq, _ptr(x), L, _ptr(prompts), P, ctypes.byref(sp),
                                     _ptr(y), _ptr(logits), _stream()), "gsv_t2s_prefill")
        return y, logits

    def t2s_decode_steps(self, steps: int, sampler: Optional[Sampler] = None, y_cap: int = 4096):
        t = self.torch
        y = t.empty((y_cap,), dtype=t.int64, device=self.dev)
        stop = t.empty((steps,), dtype=t.uint8, device=self.dev)
        logits = t.empty((steps, 1025), dtype=t.float32, device=self.dev)
        sp = sampler or make_sampler()
        _check(lib().gsv_t2s_decode_steps(self.h, 0, steps, ctypes.byref(sp), _ptr(y), _ptr(stop),
                                          _ptr(logits), _stream()), "gsv_t2s_decode_steps")
        return y, stop, logits

    def t2s_read_kv(self, layer: int, seq: int = 0, cap: int = 4096):
        t = self.torch
        k = t.empty((cap, 512), dtype=t.float32, device=self.dev)
        v = t.empty((cap, 512), dtype=t.float32, device=self.dev)
        n = ctypes.c_int32()
        _check(lib().gsv_t2s_read_kv(self.h, seq, layer, _ptr(k), _ptr(v), ctypes.byref(n),
                                     _stream()), "gsv_t2s_read_kv")
        return k[:n.value], v[:n.value]

    # -------------------------------------------------------------- VITS
    def _ids(self, x):
        t = self.torch
        return self._dev(np.asarray(x).reshape(-1) if not isinstance(x, t.Tensor) else x.reshape(-1), t.int64)

    def vits_decode(self, text_seq, pred_semantic, ref_audio=None, ge=None, ge_advanced=None,
                    eps=None, noise_scale: float = 0.5, noise_seed: Optional[int] = None, speed: float = 1.0,
                    sample_rate: Optional[int] = None, pcm16: bool = False, loudness: Optional[float] = None,
                    peak: Optional[float] = None, pause: Optional[float] = None, trim: Optional[float] = None):
        """vits_fp32.onnx for one utterance.  Noise of z_p: eps (tensor/array [192, T']) if
        given, else the engine's Philox N(0,1) stream keyed by noise_seed if given, else zeros.
        speed, sample_rate / pcm16, loudness / peak: see vocoder_options.  With an output format or
        a loudness target the result is the output stage's tensor; the 32 kHz float32 audio is
        self.vits_audio_32k[0] and the loudness stats (device float32 [4]) self.vits_loudness[0].
        pause / trim: the result is the joined sentence (vits_joined), its span self.vits_spans[0]."""
        item = dict(text_seq=text_seq, pred_semantic=pred_semantic, ref_audio=ref_audio, ge=ge,
                    ge_advanced=ge_advanced, speed=speed, sample_rate=sample_rate, pcm16=pcm16, loudness=loudness,
                    peak=peak, pause=pause, trim=trim)
        if noise_seed is not None and eps is None:
            return self.vits_decode_batch([dict(item, noise_seed=noise_seed)], noise_scale)[0]
        call = self._vocoder_call([dict(item, eps=eps)])
        _check(lib().gsv_vits_decode_item_join(self.h, call.items, call.specs, ctypes.c_float(noise_scale), _stream()),
               "gsv_vits_decode_item_join")
        return self._vits_store(call).joined(call.outs)[0]

    def audio_convert(self, audio, sample_rate: int = 32000, pcm16: bool = False, loudness: Optional[float] = None,
                      peak: Optional[float] = None, pause: Optional[float] = None, trim: Optional[float] = None):
        """The output stage alone (gsv_audio_join, whose NULL spec is gsv_audio_convert and which the
        target-only entry forwards to): 32 kHz float32 audio [n] -> its
        audio_samples(n, sample_rate) samples at sample_rate (one of SAMPLE_RATES; the polyphase
        resample of include/genie_engine.h, scipy.signal.resample_poly's default filter), as float32
        or, with pcm16, saturated int16 ((x * 32767).astype(int16), the reference's chunk format).
        One launch on the GPU; a device tensor.
        loudness / peak: the audio is first measured by ITU-R BS.1770-4 and
        every sample multiplied, before the int16 conversion, by the gain that brings it to
        `loudness` LUFS, limited so that the 32 kHz sample peak stays under `peak` (linear, None:
        -1 dBFS); self.vits_loudness[0] is then the device stats [loudness, peak, gain, blocks_kept].
        pause / trim (see vocoder_options): only the span of the audio above `trim`
        dBFS is converted and `pause` seconds of zeros follow it; self.vits_spans[0] is then the
        device span record [begin, end, n_speech, n_out] and the result has n_out samples; the
        conversion is then what vits_joined describes (vits_audio_32k stays the last vocoder call's)."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        opts = check_loudness(loudness, peak)
        opts.update(check_join(pause, trim))
        n_out = (join_samples(a.numel(), sample_rate, opts.get("pause", 0.0)) if "pause" in opts or "trim" in opts
                 else audio_samples(a.numel(), sample_rate))
        out = t.empty((n_out,), dtype=t.int16 if pcm16 else t.float32, device=self.dev)
        call = self._vocoder_specs([opts], keep=[a], outs=[out], a32=self.vits_audio_32k)
        _check(lib().gsv_audio_join(self.h, _ptr(a), a.numel(), call.specs, int(sample_rate), int(bool(pcm16)),
                                    _ptr(out), _stream()), "gsv_audio_join")
        if call.span_all is None and "pause" not in opts:   # no join option: the last call stays, but for the stats
            if call.specs is not None:
                self.vits_loudness = call.stats
            return out
        return self._vits_store(call).joined(call.outs)[0]

    def audio_loudness(self, audio):
        """(loudness in LUFS, sample peak) of 32 kHz float32 audio [n], n <= 640 * 4096, by ITU-R
        BS.1770-4 on the GPU (gsv_audio_loudness); -inf for silence.  self.vits_loudness[0] holds the
        device stats [loudness, peak, gain (1), blocks_kept]."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        stats = t.empty((4,), dtype=t.float32, device=self.dev)
        _check(lib().gsv_audio_loudness(self.h, ctypes.c_void_p(a.data_ptr()), a.numel(), _ptr(stats), _stream()),
               "gsv_audio_loudness")
        self.vits_loudness = [stats]
        lufs, pk = stats[:2].cpu().tolist()
        return lufs, pk

    def debug_join_frames(self, audio):
        """gsv_debug_join_frames: the sum of squares of each 10 ms frame (the last may be partial),
        device float64 [ceil(n / 320)]."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        e = t.empty(((a.numel() + JOIN_FRAME - 1) // JOIN_FRAME,), dtype=t.float64, device=self.dev)
        _check(lib().gsv_debug_join_frames(self.h, _ptr(a), a.numel(), _ptr(e), _stream()), "gsv_debug_join_frames")
        return e

    def debug_loudness_hops(self, audio):
        """gsv_debug_loudness_hops: the K-weighted energy of each full 100 ms hop, device [n // 3200]."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        e = t.empty((a.numel() // 3200,), dtype=t.float32, device=self.dev)
        _check(lib().gsv_debug_loudness_hops(self.h, ctypes.c_void_p(a.data_ptr()), a.numel(), _ptr(e), _stream()),
               "gsv_debug_loudness_hops")
        return e

    vits_audio_32k: list = []      # the 32 kHz float32 tensors of the last vocoder call, in item order
    vits_loudness: list = []       # its items' loudness stats (device float32 [4]; None: not normalised)
    vits_spans: list = []          # its items' span records (device int32 [4]; None: not trimmed)
    _vits_call = None              # the last call itself (VocoderCall), which the three above are read from
    _vits_async_call = None        # the overlapped single call in flight (held until vits_wait)
    _vits_batch_calls = None       # the overlapped batch in flight and the one before it (until vits_batch_wait)

    def _vits_store(self, call: VocoderCall) -> VocoderCall:
        """Make `call` the last vocoder call: vits_joined and the three lists above describe it."""
        self._vits_call = call
        self.vits_audio_32k, self.vits_loudness, self.vits_spans = call.a32, call.stats, call.spans
        return call

    def vits_joined(self, outs: Sequence):
        """The results of the last vocoder call (after its wait) cut to their joined lengths
        (VocoderCall.joined)."""
        return list(outs) if self._vits_call is None else self._vits_call.joined(outs)

    def _vocoder_specs(self, opts: Sequence[dict], keep: list, outs: list, a32: list, items=None) -> VocoderCall:
        """The VocoderCall of buffers already made, from their resolved options (vocoder_options):
        the gsv_join array beside them -- None (NULL: the plain call) when no item has a loudness
        target, a pause or a trim, else one entry per item, all zero for an item without options.
        The stats of the items with a target are device float32 [4] tensors; the span records of
        the items that trim are rows of one device int32 tensor, so joined() reads them in a single
        copy."""
        t = self.torch
        stats, spans, span_all = [None] * len(opts), [None] * len(opts), None
        if not any("loudness" in o or "pause" in o or "trim" in o for o in opts):
            return VocoderCall(items, None, keep, outs, a32, stats, spans, None)
        rows = [i for i, o in enumerate(opts) if "trim" in o]
        if rows:
            span_all = t.empty((len(rows), 4), dtype=t.int32, device=self.dev)
            for r, i in enumerate(rows):
                spans[i] = span_all[r]
        specs = (Join * len(opts))()
        for i, (j, o) in enumerate(zip(specs, opts)):
            if "loudness" in o:
                stats[i] = t.empty((4,), dtype=t.float32, device=self.dev)
                j.target, j.peak, j.stats = o["loudness"], o.get("peak", 0.0), stats[i].data_ptr()
            if "pause" in o:
                j.pause = o["pause"]
            if "trim" in o:
                j.trim, j.span = o["trim"], spans[i].data_ptr()
        return VocoderCall(items, specs, keep, outs, a32, stats, spans, span_all)

    def _vocoder_call(self, items: Sequence[dict]) -> VocoderCall:
        """One vocoder call over item dicts (text_seq, pred_semantic, ref_audio or ge + ge_advanced,
        optional eps or noise_seed, and the option keys of vocoder_options, resolved here): the
        VitsItem array, its gsv_join array (_vocoder_specs) and every tensor they point at.  With
        sample_rate / pcm16 / loudness / pause / trim an item's result is the output stage's tensor
        (its `out`); the 32 kHz float32 audio is written as well."""
        t = self.torch
        arr = (VitsItem * len(items))()
        all_opts, keep, outs, a32 = [], [], [], []
        for i, it in enumerate(items):
            opts = vocoder_options(*(it.get(k) for k in VOCODER_OPTIONS))
            ts, sem = self._ids(it["text_seq"]), self._ids(it["pred_semantic"])
            G = sem.numel()
            ra, g, ga = it.get("ref_audio"), it.get("ge"), it.get("ge_advanced")
            ra = None if ra is None else self._dev(ra, t.float32).reshape(-1)
            g = None if g is None else self._dev(g, t.float32).reshape(-1)
            ga = None if ga is None else self._dev(ga, t.float32).reshape(-1)
            speed = opts.get("speed", 1.0)
            frames = vits_frames(G, speed)
            e = it.get("eps")
            e = None if e is None else self._dev(e, t.float32).reshape(192, frames)
            seed = it.get("noise_seed")
            mode = 1 if e is not None else (2 if seed is not None else 0)
            audio = t.empty((640 * frames,), dtype=t.float32, device=self.dev)
            item = VitsItem(ts.data_ptr(), ts.numel(), sem.data_ptr(), G, 0 if ra is None else ra.data_ptr(),
                            0 if ra is None else ra.numel(), 0 if g is None else g.data_ptr(),
                            0 if ga is None else ga.data_ptr(), 0 if e is None else e.data_ptr(),
                            int(seed or 0) & 0xFFFFFFFFFFFFFFFF, mode, audio.data_ptr(), speed)
            out = audio
            if not opts.keys() <= {"speed"}:
                rate, pcm = opts.get("sample_rate", 32000), "pcm16" in opts
                n_out = (join_samples(640 * frames, rate, opts.get("pause", 0.0)) if "pause" in opts or "trim" in opts
                         else audio_samples(640 * frames, rate))
                out = t.empty((n_out,), dtype=t.int16 if pcm else t.float32, device=self.dev)
                item.out_rate, item.out_format, item.out = rate, int(pcm), out.data_ptr()
            arr[i] = item
            all_opts.append(opts)
            keep += [ts, sem, ra, g, ga, e]
            outs.append(out)
            a32.append(audio)
        return self._vocoder_specs(all_opts, keep, outs, a32, arr)

    def _vits_item(self, it: dict):
        """(VitsItem, what keeps its tensors alive, result tensor) of one item dict, for a direct call
        of a plain C entry: a _vocoder_call of it alone (the call itself is the keeper).  An item with
        a loudness target, a pause or a trim has no plain form: EngineError."""
        call = self._vocoder_call([it])
        if call.specs is not None:
            raise EngineError("loudness / pause / trim need the spec beside the item: use _vocoder_call")
        return call.items[0], call, call.outs[0]

    @staticmethod
    def vits_frames(n_sem: int, speed: float = 1.0) -> int:
        """Frames of the vocoder at this speech rate (module-level vits_frames)."""
        return vits_frames(n_sem, speed)

    def vits_decode_batch(self, items: Sequence[dict], noise_scale: float = 0.5):
        """Several vocoder calls at once (concurrent engine lanes).  Each item: text_seq,
        pred_semantic, and ref_audio (V2) or ge + ge_advanced (V2ProPlus); optional eps or
        noise_seed, and the option keys of vocoder_options.  Returns one audio tensor [640 T'] per
        item (1280 G at speed 1), the output stage's where the item asks for it (one stage launch
        for the batch); self.vits_audio_32k then holds every item's 32 kHz audio."""
        call = self._vocoder_call(items)
        _check(lib().gsv_vits_decode_batch_join(self.h, len(items), call.items, call.specs, ctypes.c_float(noise_scale),
                                                _stream()), "gsv_vits_decode_batch_join")
        return self._vits_store(call).joined(call.outs)

    def vits_decode_batch_async(self, items: Sequence[dict], noise_scale: float = 0.5):
        """vits_decode_batch without the join (gsv_vits_decode_batch_async): the lanes run
        beside whatever T2S is issued next.  Returns the audio tensors, valid after
        vits_batch_wait(); with `trim`, vits_joined(them) then cuts them to their joined lengths."""
        call = self._vocoder_call(items)
        _check(lib().gsv_vits_decode_batch_async_join(self.h, len(items), call.items, call.specs,
                                                      ctypes.c_float(noise_scale), _stream()),
               "gsv_vits_decode_batch_async_join")
        # items and device buffers live until the wait -- also a previous batch's, which this
        # call only ordered behind the engine stream (its lanes may still read them)
        # (one generation back: a batch older than the previous one was joined by this launch)
        prev = self._vits_batch_calls
        self._vits_batch_calls = (self._vits_store(call), prev and prev[0])
        return call.outs

    def vits_batch_wait(self):
        """Finish the pending vits_decode_batch_async; orders the current stream after it."""
        _check(lib().gsv_vits_batch_wait(self.h, _stream()), "gsv_vits_batch_wait")
        self._vits_batch_calls = None

    vocoder_cus = 0

    def set_vocoder_cus(self, k: int):
        """Reserve k CUs for the overlapped vocoder (0: off; see gsv_vits_decode_async)."""
        self.set_option("vocoder_cus", k)
        self.vocoder_cus = int(k)

    def vits_decode_async(self, item: dict, noise_scale: float = 0.5):
        """Start one vocoder call on the vocoder CUs (gsv_vits_decode_async) and return its
        audio tensor [640 T'], valid after vits_wait().  item as for vits_decode_batch."""
        call = self._vocoder_call([item])
        _check(lib().gsv_vits_decode_async_join(self.h, call.items, call.specs, ctypes.c_float(noise_scale), _stream()),
               "gsv_vits_decode_async_join")
        self._vits_async_call = self._vits_store(call)   # device inputs stay alive until the call is finished
        return call.outs[0]

    def vits_wait(self):
        """Finish the pending vits_decode_async call; orders the current stream after it."""
        _check(lib().gsv_vits_wait(self.h, _stream()), "gsv_vits_wait")
        self._vits_async_call = None

    def ref_encode(self, ref_audio):
        """V2: the vocoder's reference branch alone (gsv_ref_encode) -> ge [512] on the device;
        pass it as ge= (without ref_audio) to every vocoder call against this reference."""
        t = self.torch
        ra = self._dev(ref_audio, t.float32).reshape(-1)
        ge = t.empty((512,), dtype=t.float32, device=self.dev)
        _check(lib().gsv_ref_encode(self.h, _ptr(ra), ra.numel(), _ptr(ge), _stream()), "gsv_ref_encode")
        return ge

    def prompt_encode(self, ref_audio, sv_emb):
        t = self.torch
        ra = self._dev(ref_audio, t.float32).reshape(-1)
        sv = self._dev(sv_emb, t.float32).reshape(-1)
        ge = t.empty((1024,), dtype=t.float32, device=self.dev)
        ga = t.empty((512,), dtype=t.float32, device=self.dev)
        _check(lib().gsv_prompt_encode(self.h, _ptr(ra), ra.numel(), _ptr(sv), _ptr(ge), _ptr(ga),
                                       _stream()), "gsv_prompt_encode")
        return ge, ga

    def ge_mix(self, ges, weights, out=None):
        """Timbre fusion (gsv_ge_mix): device embeddings ges[i] [dim] (ref_encode's, or
        prompt_encode's ge) and their float32 weights, as mix_weights returns them -> the device
        tensor sum_i weights[i] * ges[i], one float32 chain per element in clip order with every
        multiply and add rounded on its own.  One launch.  out: the result tensor, which may be one
        of ges.  EngineError for what the entry rejects (n outside 1 .. MIX_MAX, a negative or
        non-finite weight, no weight above 0), before any launch."""
        t = self.torch
        xs = [self._dev(g, t.float32).reshape(-1) for g in ges]
        dim = xs[0].numel() if xs else 0
        if any(x.numel() != dim for x in xs):
            raise ValueError("ge_mix: embeddings of different sizes")
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if w.size != len(xs):
            raise ValueError("ge_mix: one weight per embedding")
        if out is None:
            out = t.empty((dim,), dtype=t.float32, device=self.dev)
        ptrs = (ctypes.c_void_p * max(len(xs), 1))(*[x.data_ptr() for x in xs])
        _check(lib().gsv_ge_mix(self.h, len(xs), dim, ptrs, w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                _ptr(out), _stream()), "gsv_ge_mix")
        return out

    def ge_project(self, ge):
        """V2ProPlus: ge [1024] -> ge_advanced [512] = ge_to512(ge) on the device (gsv_ge_project, the
        last step of prompt_encode alone: prompt_encode's ge gives its ge_advanced bit for bit).  The
        ge_advanced of a fused voice is this projection of the mixed ge."""
        t = self.torch
        g = self._dev(ge, t.float32).reshape(-1)
        if g.numel() != 1024:
            raise ValueError("ge_project: ge has 1024 values")
        ga = t.empty((512,), dtype=t.float32, device=self.dev)
        _check(lib().gsv_ge_project(self.h, _ptr(g), _ptr(ga), _stream()), "gsv_ge_project")
        return ga

    def hubert(self, audio_16k):
        """CN-HuBERT (gsv_hubert): raw 16 kHz audio [N] -> ssl_content [768, T] on the device."""
        t = self.torch
        a = self._dev(audio_16k, t.float32).reshape(-1)
        T = lib().gsv_hubert_frames(a.numel())
        if T < 1:
            raise EngineError(f"audio of {a.numel()} samples is too short for CN-HuBERT")
        out = t.empty((768, T), dtype=t.float32, device=self.dev)
        _check(lib().gsv_hubert(self.h, _ptr(a), a.numel(), _ptr(out), _stream()), "gsv_hubert")
        return out

    def sv(self, audio_16k):
        """Speaker verification (gsv_sv): 16 kHz audio [N] -> sv_emb [1, 20480] on the device."""
        t = self.torch
        a = self._dev(audio_16k, t.float32).reshape(-1)
        if lib().gsv_sv_frames(a.numel()) < 1:
            raise EngineError(f"audio of {a.numel()} samples is too short for the SV fbank (400 needed)")
        out = t.empty((1, 20480), dtype=t.float32, device=self.dev)
        _check(lib().gsv_sv(self.h, _ptr(a), a.numel(), _ptr(out), _stream()), "gsv_sv")
        return out

    def roberta(self, input_ids, repeats, attention_mask=None):
        """RoBERTa (gsv_roberta): token ids [N] (CLS .. SEP), word2ph [n_chars] ->
        text_bert [sum(word2ph), 1024] on the device."""
        t = self.torch
        ids = self._dev(np.asarray(input_ids).reshape(-1) if not isinstance(input_ids, t.Tensor)
                        else input_ids.reshape(-1), t.int64)
        rep = np.ascontiguousarray(np.asarray(repeats, np.int64).reshape(-1))
        mask = None if attention_mask is None else np.ascontiguousarray(np.asarray(attention_mask, np.int64).reshape(-1))
        out = t.empty((int(rep.sum()), 1024), dtype=t.float32, device=self.dev)
        _check(lib().gsv_roberta(self.h, _ptr(ids), None if mask is None else mask.ctypes.data_as(ctypes.c_void_p),
                                 ids.numel(), rep.ctypes.data_as(ctypes.c_void_p), rep.size, _ptr(out), _stream()),
               "gsv_roberta")
        return out

    def roberta_batch(self, sentences):
        """Packed RoBERTa over several sentences (gsv_roberta_batch): sentences = [(input_ids
        [N_i] CLS .. SEP, word2ph [C_i])] -> one text_bert tensor [sum(word2ph_i), 1024] per
        sentence (views of one device buffer), identical to per-sentence roberta()."""
        t = self.torch
        ids = [self._ids(i) for i, _ in sentences]          # host arrays or device tensors
        reps = [np.asarray(r, np.int64).reshape(-1) for _, r in sentences]
        dids = t.cat(ids) if len(ids) > 1 else ids[0]
        nt = np.asarray([i.numel() for i in ids], np.int32)
        nc = np.asarray([r.size for r in reps], np.int32)
        rep = np.ascontiguousarray(np.concatenate(reps)) if sum(r.size for r in reps) else np.zeros(1, np.int64)
        rows = [int(r.sum()) for r in reps]
        out = t.empty((max(1, sum(rows)), 1024), dtype=t.float32, device=self.dev)
        _check(lib().gsv_roberta_batch(self.h, len(sentences), _ptr(dids), nt.ctypes.data_as(ctypes.c_void_p),
                                       rep.ctypes.data_as(ctypes.c_void_p), nc.ctypes.data_as(ctypes.c_void_p),
                                       _ptr(out), _stream()), "gsv_roberta_batch")
        offs = np.concatenate([[0], np.cumsum(rows)])
        return [out[offs[i]:offs[i + 1]] for i in range(len(sentences))]

    def debug_copy(self, name: str, n: int):
        t = self.torch
        out = t.empty((n,), dtype=t.float32, device=self.dev)
        _check(lib().gsv_debug_copy(self.h, name.encode(), _ptr(out), n, _stream()), "gsv_debug_copy")
        return out

    def probe(self, which: int, batch: int = 1, iters: int = 200) -> float:
        """Average microseconds per launch of one kernel configuration (see gsv_probe)."""
        us = ctypes.c_float()
        _check(lib().gsv_probe(self.h, which, batch, iters, ctypes.byref(us), _stream()), "gsv_probe")
        return us.value

    def set_timing(self, on: bool = True):
        _check(lib().gsv_set_timing(self.h, int(on)), "gsv_set_timing")

    def kernel_timing(self):
        """(average microseconds, samples) of the live-sampled dominant decode kernel."""
        us, n = ctypes.c_float(), ctypes.c_int32()
        _check(lib().gsv_get_kernel_timing(self.h, ctypes.byref(us), ctypes.byref(n)), "gsv_get_kernel_timing")
        return us.value, n.value

    def set_option(self, name: str, value: int):
        """Engine option (see gsv_set_option): "persist" decode path, "ptrace" phase stamps,
        "decode_lanes" (1: started generates one behind the other instead of on two lanes)."""
        _check(lib().gsv_set_option(self.h, name.encode(), int(value)), "gsv_set_option")

    def counter(self, name: str) -> int:
        """Engine counter (gsv_get_counter): persist_timeouts, persist1_f16_reruns, vits_f32_reruns,
        sv_f32_reruns, w16_split_tensors, persist_disabled (timeout back-off holds begun),
        persist_launches, decode_lanes (1 or 2, as configured), lane_launches_0 / lane_launches_1
        (persistent launches per decode lane), persist_hold (generates left in the current hold), stops, graph_fallbacks,
        retired_bytes (replaced device buffers not yet freed), reclaimed_bytes, reclaims."""
        v = ctypes.c_int64()
        _check(lib().gsv_get_counter(self.h, name.encode(), ctypes.byref(v)), "gsv_get_counter")
        return v.value

    def ptrace(self) -> np.ndarray:
        """[256 workgroups][16 slots] stamps of the persistent decode (option ptrace):
        slots 0-7 the 100 MHz clock, 8-15 the shader clock at the same points."""
        out = np.zeros((256, 16), np.uint64)
        _check(lib().gsv_debug_ptrace(self.h, out.ctypes.data_as(ctypes.c_void_p), out.size), "gsv_debug_ptrace")
        return out

    def ktrace(self) -> np.ndarray:
        """[3 kernels][256 blocks][8 slots] realtime stamps (GENIE_KTRACE=1 builds only)."""
        out = np.zeros((3, 256, 8), np.uint64)
        _check(lib().gsv_debug_ktrace(self.h, out.ctypes.data_as(ctypes.c_void_p), out.size), "gsv_debug_ktrace")
        return out

    def timing(self) -> List[float]:
        a = (ctypes.c_float * 4)()
        _check(lib().gsv_get_timing(self.h, a), "gsv_get_timing")
        return list(a)
