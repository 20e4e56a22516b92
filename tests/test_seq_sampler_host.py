"""Host (no GPU): one sampler per sequence of a batched decode, above the kernels -- the
device entry SeqSampler and the new prototypes against the headers, Engine.t2s_generate's
argument validation, and the server's mixed_sampling rounds over a stub worker.
"""
import ctypes
import os
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the headers
def test_seq_sampler_entry_is_32_bytes_in_the_kernel_header(tmp_path):
    """SeqSampler (csrc/kernels.h), compiled alone by the host C++ compiler: 32 bytes, the
    seven fields at the offsets the kernels' one uniform read assumes."""
    src = open(os.path.join(ROOT, "genie_tts_amd", "csrc", "kernels.h")).read()
    m = re.search(r"struct SeqSampler \{.*?\};", src, re.S)
    assert m, "SeqSampler not in kernels.h"
    for name in ("SampleArgs", "PersistArgs"):
        body = re.search(r"struct %s \{.*?\n\};" % name, src, re.S).group(0)
        assert "const SeqSampler* per;" in body, name
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    prog = tmp_path / "entry.cc"
    prog.write_text("#include <cstdio>\n#include <cstddef>\n#include <cstdint>\n" + m.group(0) + "\n"
                    "int main() {\n"
                    '    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(SeqSampler), offsetof(SeqSampler, top_k),\n'
                    "                offsetof(SeqSampler, temperature), offsetof(SeqSampler, rep_penalty),\n"
                    "                offsetof(SeqSampler, top_p), offsetof(SeqSampler, greedy), offsetof(SeqSampler, stream),\n"
                    "                offsetof(SeqSampler, seed));\n    return 0;\n}\n")
    exe = tmp_path / "entry"
    subprocess.run([cxx, "-std=c++17", str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [32, 0, 4, 8, 12, 16, 20, 24]


def test_new_prototypes_are_in_the_c_header_and_the_binding(tmp_path):
    """gsv_t2s_generate_each / gsv_debug_sample_each: declared with the argument lists the
    binding passes (a C program taking their addresses through typed pointers compiles), listed
    in EXPORTED, and gsv_sampler / gsv_t2s_generate are as before."""
    from genie_tts_amd import engine as E
    assert {"gsv_t2s_generate_each", "gsv_debug_sample_each"} <= set(E.EXPORTED)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "proto.c"
    src.write_text('#include "genie_engine.h"\n'
                   "typedef int (*each_fn)(gsv_engine*, int, const gsv_utt*, const gsv_sampler*, const int32_t*,\n"
                   "                       int64_t*, int32_t, int32_t*, void*);\n"
                   "typedef int (*dbg_fn)(const float*, const uint32_t*, int, const gsv_sampler*, const int32_t*, int,\n"
                   "                      int64_t*, uint8_t*, void*);\n"
                   "typedef int (*gen_fn)(gsv_engine*, int, const gsv_utt*, const gsv_sampler*, int64_t*, int32_t,\n"
                   "                      int32_t*, void*);\n"
                   "each_fn a = gsv_t2s_generate_each;\ndbg_fn b = gsv_debug_sample_each;\ngen_fn c = gsv_t2s_generate;\n"
                   "_Static_assert(sizeof(gsv_sampler) == 40, \"gsv_sampler keeps its layout\");\n")
    subprocess.run([cc, "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "proto.o")], check=True)
    assert ctypes.sizeof(E.Sampler) == 40


# ------------------------------------------------------------------ Engine.t2s_generate's arguments
class _Lib:
    """Stands in for the shared library: records the generate calls."""

    def __init__(self):
        self.calls = []

    def gsv_t2s_generate(self, h, n, arr, sp, out, stride, lens, stream):
        self.calls.append(("one", n, None, None))
        return 0

    def gsv_t2s_generate_each(self, h, n, arr, sarr, starr, out, stride, lens, stream):
        self.calls.append(("each", n, [(s.top_k, s.seed) for s in sarr], None if starr is None else list(starr)))
        return 0


def _engine(monkeypatch):
    from genie_tts_amd import engine as E
    L = _Lib()
    monkeypatch.setattr(E, "lib", lambda: L)
    monkeypatch.setattr(E, "_stream", lambda: None)
    eng = E.Engine.__new__(E.Engine)
    eng.h = None
    monkeypatch.setattr(eng, "make_utt", lambda *u: (E.Utt(), None), raising=False)
    return E, eng, L


def test_t2s_generate_validates_samplers_and_streams(monkeypatch):
    E, eng, L = _engine(monkeypatch)
    T = [E.make_sampler(top_k=3 + i, greedy=False, seed=10 + i) for i in range(3)]
    utts = [(None,) * 5] * 3
    bads = [dict(samplers=T[:2]), dict(samplers=T + T[:1]), dict(samplers=T, streams=[0, 1]),
            dict(samplers=T, streams=[0, -1, 2]), dict(samplers=T, streams=[0, 1.5, 2]),
            dict(samplers=T, streams=[0, 1, 1 << 31]), dict(streams=[0, 1, 2]),
            dict(samplers=[T[0], None, T[2]]), dict(samplers=T, sampler=T[0])]
    for bad in bads:
        sampler = bad.pop("sampler", None)
        with pytest.raises(ValueError):
            eng.t2s_generate(utts, sampler, **bad)
    assert L.calls == []                                           # nothing reached the library
    eng.t2s_generate(utts, samplers=T, streams=[0, 0, 7])
    assert L.calls[-1] == ("each", 3, [(3, 10), (4, 11), (5, 12)], [0, 0, 7])
    eng.t2s_generate(utts, samplers=T)
    assert L.calls[-1] == ("each", 3, [(3, 10), (4, 11), (5, 12)], None)
    eng.t2s_generate(utts, T[0])                                   # the plain form is today's call
    assert L.calls[-1][0] == "one"


def test_t2s_generate_chunks_slice_both_lists(monkeypatch):
    E, eng, L = _engine(monkeypatch)
    n = E.MAX_BATCH + 6
    T = [E.make_sampler(top_k=1 + i % 60, greedy=False, seed=i) for i in range(n)]
    utts = [(None,) * 5] * n
    assert len(eng.t2s_generate(utts, samplers=T, streams=list(range(100, 100 + n)))) == n
    (k0, n0, s0, st0), (k1, n1, s1, st1) = L.calls
    assert (k0, n0, k1, n1) == ("each", E.MAX_BATCH, "each", 6)
    assert [s for _, s in s0 + s1] == list(range(n)) and st0 + st1 == list(range(100, 100 + n))
    L.calls.clear()
    eng.t2s_generate(utts, samplers=T)                             # streams None: each chunk numbers from 0
    assert [c[3] for c in L.calls] == [None, None]
    with pytest.raises(ValueError):
        eng.t2s_generate(utts, samplers=T[:-1])                    # the whole list is checked before any chunk
    assert len(L.calls) == 2


def test_tts_batch_t2s_passes_the_lists_through():
    from types import SimpleNamespace
    from genie_tts_amd.engine import make_sampler
    from genie_tts_amd.inference import GENIE
    calls = []

    class Eng:
        def t2s_generate(self, utts, sampler=None, out_stride=1024, **kw):
            calls.append((len(utts), sampler, kw))
            return [np.zeros(3, np.int64)] * len(utts)
    model = SimpleNamespace(ENGINE=Eng())
    ref = SimpleNamespace(ssl_content=np.zeros((768, 4), np.float32), phonemes_seq=np.arange(3), text_bert=None)
    items = [(np.arange(4), None, 5), (np.arange(5), None)]
    own = make_sampler()
    T = [make_sampler(greedy=False, seed=1), make_sampler(greedy=False, seed=2)]
    g = GENIE()
    g.tts_batch_t2s(items, ref, model, own)
    assert calls[-1] == (2, own, {})                               # without the new arguments: today's call
    g.tts_batch_t2s(items, ref, model, own, samplers=T, streams=[0, 1])
    assert calls[-1] == (2, None, dict(samplers=T, streams=[0, 1]))


# ------------------------------------------------------------------ the server
def _worker(monkeypatch, own, gate=None, mixed=True):
    """tests/test_top_p_host.py's stub worker with cfg["mixed_sampling"]; rounds holds
    (batch size, sampler, samplers, streams) of every generate."""
    import multiprocessing as mp
    from genie_tts_amd import api
    from genie_tts_amd.inference import tts_client
    from genie_tts_amd.model_manager import model_manager
    from genie_tts_amd.server import _worker_main

    class M:
        LANGUAGE = "Japanese"
        ENGINE = None
        VITS = None
        T2S_FIRST_STAGE_DECODER = type("D", (), {"sampler": own})()

    rounds = []

    def t2s(items, ref, m, sp, samplers=None, streams=None):
        if gate is not None:
            assert gate.wait(60)
        rounds.append((len(items), sp, samplers, streams))
        return [None] * len(items)
    model = M()
    monkeypatch.setattr(model_manager, "get", lambda name: model)
    monkeypatch.setitem(api._reference_audios, "a", object())
    monkeypatch.setattr(tts_client, "tts_batch_t2s", t2s)
    monkeypatch.setattr(tts_client, "tts_batch_vocoder",
                        lambda items, toks, ref, m, overlapped=False, speed=1.0: [np.zeros(640, np.float32)] * len(items))
    parent, child = mp.Pipe()
    cfg = {"g2p": "genie_tts_amd.stubs:toy_g2p", "mixed_sampling": mixed}
    t = threading.Thread(target=_worker_main, args=(0, child, cfg), daemon=True)
    t.start()
    assert parent.poll(60) and parent.recv()["kind"] == "ready"
    return parent, t, rounds


def test_mixed_rounds_take_every_ready_request(monkeypatch):
    """The five-request burst of test_top_p_host.test_rounds_group_by_sampler, held behind the
    gate (request 0's round waits in the stub until the burst is sent): with mixed_sampling
    it goes out as ONE round with five samplers and streams."""
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    from tests.test_top_p_host import _collect
    own = make_sampler(greedy=False, seed=1)
    gate = threading.Event()
    parent, t, rounds = _worker(monkeypatch, own, gate)
    try:
        parent.send(dict(cmd="tts", id=0, character_name="a", text="かき。"))
        burst = ((1, dict(top_p=0.5)), (2, dict(top_p=0.9, seed=77)), (3, dict(top_p=0.5)), (4, {}),
                 (5, dict(top_k=own.top_k, seed=5)))
        for rid, kw in burst:
            parent.send(dict(cmd="tts", id=rid, character_name="a", text="かき。", **kw))
        gate.set()
        got = _collect(parent, [0, 1, 2, 3, 4, 5])
        assert all(v == ["chunk", "end"] for v in got.values()), got
        # request 0 may have begun its round alone before the burst arrived; the burst itself
        # is one round either way (in the other order all six share the first round)
        assert [r[0] for r in rounds] in ([1, 5], [6]), [r[0] for r in rounds]
        n, sp, each, streams = rounds[-1]
        assert sp is None and len(each) == n and len(streams) == n
        each, streams = each[-5:], streams[-5:]
        pos = list(range(n - 5, n))
        assert [round(float(s.top_p), 3) for s in each] == [0.5, 0.9, 0.5, 1.0, 1.0]
        assert [s.seed for s in each] == [1, 77, 1, 1, 5]
        assert each[3] is own                                      # no control: the character's own
        assert all(s is not own for s in each[:3])
        assert streams == [pos[0], 0, pos[2], pos[3], 0]           # a given seed: stream 0; else the position
        assert own.top_p == 1.0 and own.seed == 1
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)


def test_mixed_rounds_a_bad_control_ends_only_its_request(monkeypatch):
    from genie_tts_amd import api
    from genie_tts_amd.engine import make_sampler
    from tests.test_top_p_host import _collect
    own = make_sampler(greedy=False, seed=1)
    parent, t, rounds = _worker(monkeypatch, own)
    try:
        parent.send(dict(cmd="tts", id=1, character_name="a", text="かき。", top_p=1.5))
        got = _collect(parent, [1])[1]
        assert len(got) == 1 and got[0][0] == "error" and got[0][1].startswith("sampling:") and "top_p" in got[0][1]
        assert rounds == []
        parent.send(dict(cmd="tts", id=2, character_name="a", text="かき。", top_k=4))
        assert _collect(parent, [2])[2] == ["chunk", "end"]
        assert rounds[-1][0] == 1 and rounds[-1][2][0].top_k == 4 and rounds[-1][3] == [0]
    finally:
        parent.send(None)
        t.join(timeout=30)
        api.set_g2p(None)


def test_router_and_command_line_carry_the_switch():
    import inspect
    from genie_tts_amd import server
    assert server.Router([0], worker=lambda *a: None).cfg["mixed_sampling"] is False
    assert server.Router([0], worker=lambda *a: None, mixed_sampling=True).cfg["mixed_sampling"] is True
    assert inspect.signature(server.start_server).parameters["mixed_sampling"].default is False
    assert "--mixed-sampling" in inspect.getsource(server)
