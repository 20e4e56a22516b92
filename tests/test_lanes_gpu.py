"""GPU: the decode lanes (option "decode_lanes") -- under option vocoder_cus with >= 192 decode
CUs, two started generates (gsv_t2s_generate_start) decode side by side, each on its own half of
the decode CUs with a KV slot, hand-off ring and error word of its own.

Bars: every token list identical to the plain gsv_t2s_generate of that sentence alone (greedy
and top-k sampled: a lane's prefill and decode draw sequence 0's Philox noise), whichever lane
it ran on and whether it was prefetched or prefilled itself; the counters show that both lanes
really launched; no persistent-decode timeout; the overlapped vocoder beside them is bit-equal to
the sequential one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
STEPS = (20, 6, 14, 6, 20, 9)   # unequal: sentence 1 finishes before sentence 0, 3 before 2


@pytest.fixture(scope="module")
def eng():
    from genie_tts_amd import synth
    from genie_tts_amd.engine import Engine
    w = synth.synthetic_character("v2")
    e = Engine({k: w[k] for k in w}, "v2", pe_div_term=np.load(os.path.join(GOLD, "pe_div_term.npy")))
    e.set_option("persist", 1)
    yield e
    e.set_vocoder_cus(0)
    e.close()


@pytest.fixture(scope="module")
def sentences(eng):
    """Six distinct sentences as device-resident utterance tuples with their own force_steps."""
    from tests.common import t2s_inputs
    out = []
    for i, n in enumerate(STEPS):
        u = t2s_inputs(R=11 + (3 * i) % 9, S=9 + (7 * i) % 17, H=33 + (13 * i) % 41, tag=f"ln{i}", bert=i % 2 == 1)
        out.append(tuple(eng._dev(a, None) for a in u) + (n,))
    return out


@pytest.fixture(scope="module")
def plain(eng, sentences):
    """The plain path, computed once: {greedy: token lists} of every sentence alone, no CU split."""
    eng.set_vocoder_cus(0)
    return {g: [eng.t2s_generate([u], sampler(g))[0].tolist() for u in sentences] for g in (True, False)}


def sampler(greedy):
    from genie_tts_amd.engine import make_sampler
    return make_sampler(greedy=True) if greedy else make_sampler(top_k=5, greedy=False, seed=1234)


def lane_counters(eng):
    return [eng.counter(n) for n in ("lane_launches_0", "lane_launches_1", "persist_timeouts", "persist1_f16_reruns")]


def run_stream(eng, utts, sp, prefetch=True):
    """bench.py's Runner.stream call pattern: prefetch i+2, start i+1, finish i."""
    n = len(utts)
    if prefetch and n > 1:
        eng.t2s_prefetch(utts[1], sp)
    eng.t2s_generate_start(utts[0], sp)
    got = []
    for i in range(n):
        if i + 1 < n:
            if prefetch and i + 2 < n:
                eng.t2s_prefetch(utts[i + 2], sp)
            eng.t2s_generate_start(utts[i + 1], sp)
        got.append(eng.t2s_generate_finish().tolist())
    return got


@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("prefetch", [True, False])
def test_two_lane_stream_matches_plain(eng, sentences, plain, greedy, prefetch):
    """With and without prefetches (every start then prefills itself on its lane while the other
    lane decodes): exact, three launches on each lane."""
    eng.set_vocoder_cus(64)
    try:
        assert eng.counter("decode_lanes") == 2
        c0 = lane_counters(eng)
        got = run_stream(eng, sentences, sampler(greedy), prefetch)
        c1 = lane_counters(eng)
        for i, (a, b) in enumerate(zip(got, plain[greedy])):
            assert a == b, f"sentence {i}"
        assert [c1[0] - c0[0], c1[1] - c0[1]] == [3, 3]
        assert c1[2:] == c0[2:]
    finally:
        eng.set_vocoder_cus(0)


def test_two_lanes_fp16_guard_reruns_both(eng, sentences, plain):
    """Both launches in flight meet the (test-lowered) fp16 limit: each is re-run synchronously
    inside its _finish, and the second one's state survives the first one's re-run."""
    sp = sampler(True)
    eng.set_vocoder_cus(64)
    n0 = eng.counter("persist1_f16_reruns")
    eng.set_option("persist1_f16_limit", 1)
    try:
        eng.t2s_generate_start(sentences[0], sp)
        eng.t2s_generate_start(sentences[1], sp)
        assert eng.t2s_generate_finish().tolist() == plain[True][0]
        assert eng.t2s_generate_finish().tolist() == plain[True][1]
    finally:
        eng.set_option("persist1_f16_limit", 0)
        eng.set_vocoder_cus(0)
    assert eng.counter("persist1_f16_reruns") >= n0 + 2


@pytest.mark.parametrize("lanes,K", [(1, 64), (2, 96)])
def test_one_lane_where_asked_or_where_two_do_not_fit(eng, sentences, plain, lanes, K):
    """Option decode_lanes = 1, and K = 96 (160 decode CUs): one lane, the second start queued
    behind the first on the engine stream as before."""
    sp = sampler(False)
    eng.set_option("decode_lanes", lanes)
    eng.set_vocoder_cus(K)
    try:
        assert eng.counter("decode_lanes") == 1
        c0 = lane_counters(eng)
        got = run_stream(eng, sentences[:4], sp)
        c1 = lane_counters(eng)
        assert got == plain[False][:4]
        assert c1[0] - c0[0] == 4 and c1[1] == c0[1]
        assert c1[2] == c0[2]
    finally:
        eng.set_vocoder_cus(0)
        eng.set_option("decode_lanes", 2)


def test_two_lanes_on_224_decode_cus(eng, sentences, plain):
    """K = 32: lanes of 128 + 96 CUs."""
    eng.set_vocoder_cus(32)
    try:
        assert eng.counter("decode_lanes") == 2
        c0 = lane_counters(eng)
        got = run_stream(eng, sentences, sampler(True))
        c1 = lane_counters(eng)
        assert got == plain[True]
        assert [c1[0] - c0[0], c1[1] - c0[1]] == [3, 3]
        assert c1[2] == c0[2]
    finally:
        eng.set_vocoder_cus(0)


def test_overlapped_vocoder_beside_two_lanes(eng, sentences, plain):
    """Runner.stream's interleaving: sentence i's vocoder queued behind its finish, launched on
    the vocoder CUs by the next start, beside both decode lanes.  Waveforms bit-equal to the
    sequential vocoder's."""
    import torch
    v = dict(np.load(os.path.join(GOLD, "vits_v2_g80.npz"), allow_pickle=False))
    item = dict(text_seq=v["text_seq"], pred_semantic=v["pred_semantic"], ref_audio=v["ref_audio"],
                noise_seed=int(v["noise_seed"]))
    sp = sampler(True)
    utts = sentences[:3]
    eng.set_vocoder_cus(0)
    seq_audio = eng.vits_decode(v["text_seq"], v["pred_semantic"], ref_audio=v["ref_audio"],
                                noise_seed=int(v["noise_seed"])).cpu()
    r0 = eng.counter("vits_f32_reruns")
    eng.set_vocoder_cus(64)
    try:
        c0 = lane_counters(eng)
        audios, got, pending = [], [], False
        eng.t2s_prefetch(utts[1], sp)
        eng.t2s_generate_start(utts[0], sp)
        for i in range(3):
            if i + 1 < 3:
                if i + 2 < 3:
                    eng.t2s_prefetch(utts[i + 2], sp)
                eng.t2s_generate_start(utts[i + 1], sp)
            got.append(eng.t2s_generate_finish().tolist())
            if pending:
                eng.vits_wait()
            audios.append(eng.vits_decode_async(item))
            pending = True
        eng.vits_wait()
        c1 = lane_counters(eng)
        assert got == plain[True][:3]
        for a in audios:
            assert torch.equal(a.cpu(), seq_audio)
        assert [c1[0] - c0[0], c1[1] - c0[1]] == [2, 1]
        assert c1[2] == c0[2] and eng.counter("vits_f32_reruns") == r0
    finally:
        eng.set_vocoder_cus(0)


def test_growth_while_the_other_lane_decodes(eng, sentences, plain):
    """A start that needs more tokens than reserved while the other lane is in flight: both lanes
    are drained before the KV cache is re-allocated, and both results are exact.  (Last in the
    module: the state stays grown.)"""
    from genie_tts_amd.engine import make_sampler
    sp = make_sampler(greedy=True)
    big = sentences[2][:5] + (300,)   # > the 256 tokens the sentences above reserve
    eng.set_vocoder_cus(64)
    try:
        c0 = lane_counters(eng)
        r0 = eng.counter("reclaims")
        eng.t2s_generate_start(sentences[0], sp)
        eng.t2s_generate_start(big, sp)
        assert eng.counter("reclaims") > r0   # the state was re-allocated by the second start
        got = [eng.t2s_generate_finish().tolist(), eng.t2s_generate_finish().tolist()]
        c1 = lane_counters(eng)
        assert [c1[0] - c0[0], c1[1] - c0[1]] == [1, 1]
        assert c1[2] == c0[2]
    finally:
        eng.set_vocoder_cus(0)
    assert got[0] == plain[True][0]
    assert got[1] == eng.t2s_generate([big], sp)[0].tolist()   # the plain path, after the fact
