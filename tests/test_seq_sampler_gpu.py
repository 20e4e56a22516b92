"""GPU: one sampler per sequence of a batched decode (gsv_t2s_generate_each).

The sampler kernel with a table against the host oracle (debug_sample_each), then the
generate on every decode path -- per-step graphs, k_decode_persist1m, k_decode_persistm and
the single-sequence kernel -- against plain t2s_generate runs.  Every comparison is token
equality.  Inputs: the synthetic character and t2s_inputs(R=10+3i, S=8+2i, H=30+6i), 24
forced steps per sequence.
"""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import top_p_oracle as O
from tests.philox import sampler_noise

pytestmark = pytest.mark.gpu
STEPS = 24
PATHS = ("graphs", "persist1m", "persistm")


# ------------------------------------------------------------------ the sampler kernel
def _rows(seed=4242, Bs=7):
    """tests/test_sampler_gpu.py-style rows: N(0, 3) logits with ties, a plateau and an EOS
    leader, random histories."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 3, size=(Bs, 1025)).astype(np.float32)
    logits[2, :40] = logits[2].max() + 1.0
    logits[3, 100:130] = 2.5
    logits[3, 500:505] = 9.0
    logits[4, 1024] = logits[4].max() + 5.0
    hists = [rng.choice(1025, size=int(rng.integers(0, 200)), replace=False) for _ in range(Bs)]
    return logits, hists


def _dev(logits, hists):
    import torch
    seen = np.stack([O.seen_bits(h) for h in hists])
    return torch.from_numpy(np.ascontiguousarray(logits)).cuda(), torch.from_numpy(seen).cuda()


def test_sampler_kernel_reads_its_row_of_the_table():
    """Seven rows, each with its own (top_k, temperature, repetition_penalty, top_p, greedy, seed,
    stream): every token is the oracle's, fed the Philox normals of that row's seed and stream."""
    from genie_tts_amd.engine import debug_sample_each, make_sampler
    logits, hists = _rows()
    step = 13
    rp5 = 1.2
    top_p5 = O.pick_top_p([(logits[5], hists[5])], 0.4, repetition_penalty=rp5)
    assert O.margin(logits[5], hists[5], top_p5, rp5) >= O.MARGIN
    kept = int(O.survivors(O.penalised(logits[5], hists[5], rp5), top_p5).sum())
    assert 1 <= kept < 15, kept                                  # the nucleus bites: fewer survivors than top_k
    #          top_k temp  rep   top_p  greedy seed  stream
    table = [(15,   1.0,  1.35, 1.0,   True,  0,    0),        # greedy at temperature 1
             (5,    0.7,  1.35, 1.0,   False, 11,   1),
             (64,   1.0,  1.1,  1.0,   False, 12,   9),
             (15,   1.3,  1.5,  1.0,   False, 1 << 40, 3),     # a seed beyond 32 bits
             (1,    1.0,  1.35, 1.0,   False, 14,   4),
             (15,   0.8,  rp5,  top_p5, False, 15,  5),
             (15,   0.8,  rp5,  top_p5, False, 15,  6)]         # row 5 again but for the stream
    logits[6], hists[6] = logits[5], hists[5]
    T = [make_sampler(top_k=k, temperature=t, repetition_penalty=rp, greedy=g, seed=s, top_p=p)
         for k, t, rp, p, g, s, _ in table]
    streams = [r[6] for r in table]
    tok, stop = debug_sample_each(*_dev(logits, hists), T, step, streams=streams)
    tok, stop = tok.cpu().numpy(), stop.cpu().numpy()
    for b, (k, t, rp, p, g, s, strm) in enumerate(table):
        q = np.ones(1025, np.float32) if g else sampler_noise(1025, step, strm, s)
        t_ref, raw = O.sample(logits[b], hists[b], q, k, t, repetition_penalty=rp, top_p=p)
        assert int(tok[b]) == t_ref, (b, int(tok[b]), t_ref)
        assert bool(stop[b]) == (raw == 1024 or t_ref == 1024)
    # the two rows that differ in the stream alone draw different noise (checked on the oracle's
    # tokens over a few steps, so the pair is not vacuous at this step by chance)
    differ = sum(O.sample(logits[5], hists[5], sampler_noise(1025, s, 5, 15), 15, 0.8, rp5, top_p5)[0] !=
                 O.sample(logits[5], hists[5], sampler_noise(1025, s, 6, 15), 15, 0.8, rp5, top_p5)[0]
                 for s in range(1, 9))
    assert differ >= 1
    for s in range(1, 9):
        tk, _ = debug_sample_each(*_dev(logits[5:7], hists[5:7]), T[5:7], s, streams=[5, 6])
        for j in range(2):
            assert int(tk[j]) == O.sample(logits[5], hists[5], sampler_noise(1025, s, 5 + j, 15), 15, 0.8, rp5,
                                          top_p5)[0], (s, j)


def test_table_of_equal_entries_is_debug_sample():
    from genie_tts_amd.engine import debug_sample, debug_sample_each, make_sampler
    logits, hists = _rows(77)
    lg, seen = _dev(logits, hists)
    for sp in (make_sampler(top_k=9, temperature=0.9, greedy=False, seed=5), make_sampler(greedy=True)):
        a, sa = debug_sample(lg, seen, sp, 4)
        b, sb = debug_sample_each(lg, seen, [sp] * len(hists), 4)
        assert a.tolist() == b.tolist() and sa.tolist() == sb.tolist()


# ------------------------------------------------------------------ the generate
def _new_engine():
    from genie_tts_amd.engine import Engine
    from tests.common import character
    w = character("v2")
    return Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")


@pytest.fixture(scope="module")
def eng():
    e = _new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def inps():
    from tests.common import t2s_inputs
    return [t2s_inputs(R=10 + 3 * i, S=8 + 2 * i, H=30 + 6 * i, tag=f"sq{i}") for i in range(17)]


@pytest.fixture(scope="module")
def tight(eng, inps):
    """A top_p that bites on the synthetic model's near-flat distribution, as
    tests/test_top_p_gpu.py picks it: the midpoint between the 4th and 5th cumulative
    probability of sentence 0's first-stage logits."""
    import torch
    ref, txt, rb, tb, ssl = inps[0]
    x, prompts = eng.t2s_encode(ref, txt, None, None, ssl)
    _, logits = eng.t2s_prefill(x, prompts)
    _, S = O.cum_probs(torch.as_tensor(logits.cpu().numpy()))
    return float(np.float32(0.5 * (float(S[3]) + float(S[4]))))


def _table(B, tight):
    """T: greedy | sampled, top_k 5, seed 3 | sampled, top_k 15, biting top_p, temperature 0.8,
    seed 9; repeated with other seeds for larger B."""
    from genie_tts_amd.engine import make_sampler
    T = []
    for b in range(B):
        r = b // 3
        T.append((make_sampler(greedy=True, force_steps=STEPS),
                  make_sampler(top_k=5, greedy=False, seed=3 + 100 * r, force_steps=STEPS),
                  make_sampler(top_k=15, greedy=False, seed=9 + 100 * r, temperature=0.8, top_p=tight,
                               force_steps=STEPS))[b % 3])
    return T


@contextlib.contextmanager
def _path(eng, name):
    """The decode path of generates of B >= 2 (B = 1: the single-sequence kernel, or the
    graphs); the options are restored on the way out."""
    try:
        if name == "graphs":
            eng.set_option("persist", 0)
        elif name == "persistm":
            eng.set_option("persistm", 1)
            eng.set_option("persistm_min_b", 2)
        else:
            assert name == "persist1m"
        yield
    finally:
        eng.set_option("persist", 1)
        eng.set_option("persistm_min_b", 32)


def _plain(eng, utts, sp):
    return [t.tolist() for t in eng.t2s_generate(utts, sp)]


def _each(eng, utts, T, streams=None, path=None):
    """A samplers= generate; on a persistent path: one launch, which completed (no re-run on
    the graphs, so the named kernel produced the tokens)."""
    c0 = [eng.counter(n) for n in ("persist_launches", "persist_timeouts", "persist1_f16_reruns")]
    out = [t.tolist() for t in eng.t2s_generate(utts, samplers=T, streams=streams)]
    c1 = [eng.counter(n) for n in ("persist_launches", "persist_timeouts", "persist1_f16_reruns")]
    if path is not None:
        assert c1 == [c0[0] + (path != "graphs"), c0[1], c0[2]], (path, c0, c1)
    return out


def _key(sp):
    from genie_tts_amd.engine import sampler_key
    return sampler_key(sp)


_uniform_cache = {}


def _uniform(eng, inps, tight, path, B):
    """{sampler key: rows of the plain generate of B sentences with that entry of T}, computed
    once per (path, B) and shared."""
    if (path, B) not in _uniform_cache:
        T = _table(B, tight)
        runs = {}
        with _path(eng, path):
            for sp in T:
                if _key(sp) not in runs:
                    runs[_key(sp)] = _plain(eng, inps[:B], sp)
        _uniform_cache[(path, B)] = runs
    return _uniform_cache[(path, B)]


@pytest.mark.parametrize("path,B", [("graphs", 3), ("persist1m", 3), ("persist1m", 17), ("persistm", 3),
                                    ("persistm", 5), ("persistm", 17)])
def test_mixed_table_equals_the_uniform_runs(eng, inps, tight, path, B):
    """Row b of the samplers=T generate is row b of the plain generate with T[b] (streams None:
    the slot numbering of the plain call).  B = 17: sampler workgroup h of k_decode_persist1m
    takes sequences h and h + 16; k_decode_persistm spreads B <= 16 sequences over B groups
    (B = 5: more than one group) and at B = 17 group 0 holds sequences 0 and 16 (b = g + i nsg)."""
    T = _table(B, tight)
    runs = _uniform(eng, inps, tight, path, B)
    # not vacuous: for any two distinct entries, their uniform runs differ on the rows of both
    keys = [_key(sp) for sp in T]
    for i in range(B):
        assert len(runs[keys[i]][i]) == STEPS - 1
        for j in range(i + 1, B):
            if keys[i] != keys[j]:
                assert runs[keys[i]][i] != runs[keys[j]][i] and runs[keys[i]][j] != runs[keys[j]][j], (i, j)
    with _path(eng, path):
        got = _each(eng, inps[:B], T, path=path)
    for b in range(B):
        assert got[b] == runs[keys[b]][b], (path, B, b)


def test_mixed_table_with_the_per_slot_prefill(eng, inps, tight):
    """Option packed = 0: the first-stage sampler runs once per slot (one block, b0 = slot) and
    reads the slot's entry."""
    T = _table(3, tight)
    runs = _uniform(eng, inps, tight, "persist1m", 3)
    eng.set_option("packed", 0)
    try:
        got = _each(eng, inps[:3], T, path="persist1m")
    finally:
        eng.set_option("packed", 1)
    assert got == [runs[_key(T[b])][b] for b in range(3)]


@pytest.mark.parametrize("path", PATHS)
def test_equal_entries_equal_the_plain_generate(eng, inps, tight, path):
    T = _table(3, tight)
    runs = _uniform(eng, inps, tight, path, 3)
    with _path(eng, path):
        for sp in T:
            assert _each(eng, inps[:3], [sp] * 3, path=path) == runs[_key(sp)], (path, _key(sp))


@pytest.mark.parametrize("path", ["persist1m", "persistm"])
def test_stream_zero_draws_the_single_generate(eng, inps, tight, path):
    """streams = [0] * B: every row is that sentence's own B = 1 generate with T[b] -- the
    property the server's seeded requests rest on.  (The plain call gives it for slot 0 only:
    tests/test_top_p_gpu.py::test_multi_sequence_kernel_agrees.)  Its premise, checked first: the
    path's logits equal the single-sequence kernel's at these inputs (greedy rows equal their own
    B = 1 generates)."""
    from genie_tts_amd.engine import make_sampler
    T = _table(3, tight)
    greedy = make_sampler(greedy=True, force_steps=STEPS)
    alone_greedy = [_plain(eng, [inps[b]], greedy)[0] for b in range(3)]
    alone = [_plain(eng, [inps[b]], T[b])[0] for b in range(3)]
    with _path(eng, path):
        assert _plain(eng, inps[:3], greedy) == alone_greedy          # the premise
        got = _each(eng, inps[:3], T, streams=[0, 0, 0], path=path)
        slots = _each(eng, inps[:3], T, path=path)
    assert got == alone
    assert slots[1] != alone[1] and slots[2] != alone[2]              # (the slot numbering draws other noise)


def test_single_sequence_kernel_honours_the_stream(eng, inps, tight):
    """B = 1 with streams = [2] on k_decode_persist1 (and on the graphs) is row 2 of a plain
    B = 3 generate that holds the sentence in slot 2; streams None is the plain B = 1 call."""
    sp = _table(3, tight)[1]
    want = _uniform(eng, inps, tight, "persist1m", 3)[_key(sp)][2]
    alone = _plain(eng, [inps[2]], sp)[0]
    assert want != alone
    assert _each(eng, [inps[2]], [sp], streams=[2], path="persist1")[0] == want
    assert _each(eng, [inps[2]], [sp], path="persist1")[0] == alone
    with _path(eng, "graphs"):
        assert _each(eng, [inps[2]], [sp], streams=[2], path="graphs")[0] == want


def test_step_graphs_replay_after_the_table_changes(eng, inps, tight):
    """Per-step graphs: two samplers= generates of one B with different tables, a plain
    generate, then the first table again on one engine; each equals a fresh engine's first run."""
    T1 = _table(3, tight)
    T2 = [T1[2], T1[0], T1[1]]
    with _path(eng, "graphs"):
        a1 = _each(eng, inps[:3], T1, path="graphs")
        a2 = _each(eng, inps[:3], T2, path="graphs")
        p = _plain(eng, inps[:3], T1[1])
        a3 = _each(eng, inps[:3], T1, path="graphs")
    assert a1 == a3 and a1 != a2 and p != a1 and p != a2
    for first, rest in ((("each", T2, a2), (("plain", T1[1], p),)), (("each", T1, a1), ())):
        e2 = _new_engine()
        try:
            e2.set_option("persist", 0)
            for kind, t, want in (first,) + rest:
                got = _each(e2, inps[:3], t, path="graphs") if kind == "each" else _plain(e2, inps[:3], t)
                assert got == want, kind
        finally:
            e2.close()


def test_errors_launch_nothing_and_leave_the_engine_sound(eng, inps, tight):
    import torch
    from genie_tts_amd.engine import EngineError, Sampler, lib, make_sampler
    T = _table(3, tight)
    n0 = eng.counter("persist_launches")

    def copy(sp, **kw):
        c = Sampler.from_buffer_copy(sp)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    with pytest.raises(EngineError, match=r"samplers\[2\].*top_p"):
        eng.t2s_generate(inps[:3], samplers=[T[0], T[1], copy(T[2], top_p=1.5)])
    with pytest.raises(EngineError, match=r"samplers\[1\].*top_k"):
        eng.t2s_generate(inps[:3], samplers=[T[0], copy(T[1], top_k=65), T[2]])
    with pytest.raises(EngineError, match=r"samplers\[1\].*max_steps"):
        eng.t2s_generate(inps[:3], samplers=[T[0], copy(T[1], max_steps=400), T[2]])
    with pytest.raises(ValueError, match="streams"):
        eng.t2s_generate(inps[:3], samplers=T, streams=[0, -1, 2])
    with pytest.raises(ValueError, match="samplers"):
        eng.t2s_generate(inps[:3], samplers=T[:2])
    with pytest.raises(ValueError, match="streams"):
        eng.t2s_generate(inps[:3], samplers=T, streams=[0, 1])
    # the C entry itself refuses a negative stream (the Python layer never lets one through)
    lg = torch.zeros((2, 1025), device="cuda")
    seen = torch.zeros((2, 33), dtype=torch.int32, device="cuda")
    tok = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = lib().gsv_debug_sample_each(lg.data_ptr(), seen.data_ptr(), 2, (Sampler * 2)(T[1], T[1]),
                                     (ctypes.c_int32 * 2)(0, -1), 1, tok.data_ptr(), None, None)
    assert rc != 0 and b"streams[1]" in lib().gsv_last_error()
    assert eng.counter("persist_launches") == n0
    assert _plain(eng, inps[:3], T[1]) == _uniform(eng, inps, tight, "persist1m", 3)[_key(T[1])]


def test_tts_batch_with_a_sampler_per_item(inps, tight):
    """GENIE.tts_batch of 3 items with samplers=T: each waveform has 1280 samples per semantic
    token of the same items' T2S (the tokens of the mixed-table case)."""
    from genie_tts_amd import synth
    from genie_tts_amd.engine import make_sampler
    from genie_tts_amd.inference import GENIE, ReferenceAudio
    from genie_tts_amd.model_manager import build_model
    from tests.common import character
    m = build_model(character("v2"), "v2", sampler=make_sampler(greedy=True))
    m.VITS.noise = "zero"
    try:
        ref = ReferenceAudio(phonemes_seq=synth.synth_phones(12, "sq-r"), text_bert=np.zeros((12, 1024), np.float32),
                             audio_32k=synth.synth_ref_audio(32000 * 2, "sq-a").reshape(1, -1),
                             ssl_content=synth.synth_ssl(41, "sq-s").reshape(1, 768, -1))
        items = [(synth.synth_phones(n, f"sq-t{n}"), None) for n in (10, 17, 25)]
        T = _table(3, tight)
        gen = GENIE()
        toks = gen.tts_batch_t2s(items, ref, m, None, samplers=T)
        own = [gen.tts_batch_t2s(items, ref, m, T[b])[b] for b in range(3)]
        for b in range(3):
            assert toks[b].tolist() == own[b].tolist() and toks[b].size == STEPS - 1
        assert toks[1].tolist() != gen.tts_batch_t2s(items, ref, m, T[2])[1].tolist()
        wavs = gen.tts_batch(items, ref, m, None, samplers=T)
        assert [np.asarray(w).size for w in wavs] == [1280 * t.size for t in toks]
    finally:
        m.ENGINE.close()
