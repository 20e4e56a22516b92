"""GPU: the ring depth of the small-M GEMM form (option "gemm_small_ns") -- a prefill whose
grids exceed the CUs of its stream takes a two-stage LDS ring, so three blocks share a CU
(three stages, two blocks, by the option only).  Every depth runs the same MFMA sequence and K partition.

Bars: with the depth forced to 2, 3 and 4 the tokens (greedy and top-k sampled) and the K/V
rows of layers 0 and 23 are identical; the stream call pattern under set_vocoder_cus(64) and
(8) -- where the automatic rule picks the shallow form even at these small shapes -- gives the
plain path's tokens with no persistent-decode timeout."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
STEPS = 6
# N0 = R + S + H // 2: 36 (one ragged M tile) and 81 (two tiles, the last ragged)
SHAPES = [dict(R=11, S=9, H=33), dict(R=19, S=25, H=74)]


@pytest.fixture(scope="module")
def eng():
    from genie_tts_amd import synth
    from genie_tts_amd.engine import Engine
    w = synth.synthetic_character("v2")
    e = Engine({k: w[k] for k in w}, "v2", pe_div_term=np.load(os.path.join(GOLD, "pe_div_term.npy")))
    e.set_option("persist", 1)
    yield e
    e.set_option("gemm_small_ns", 0)
    e.set_vocoder_cus(0)
    e.close()


@pytest.fixture(scope="module")
def sentences(eng):
    from tests.common import t2s_inputs
    out = []
    for i, sh in enumerate(SHAPES):
        u = t2s_inputs(tag=f"gf{i}", bert=i % 2 == 1, **sh)
        assert np.asarray(u[0]).size + np.asarray(u[1]).size + sh["H"] // 2 == (36, 81)[i]
        out.append(tuple(eng._dev(a, None) for a in u) + (STEPS,))
    return out


def sampler(greedy):
    from genie_tts_amd.engine import make_sampler
    return make_sampler(greedy=True) if greedy else make_sampler(top_k=5, greedy=False, seed=1234)


def _generate(eng, u, greedy):
    """Tokens and the K/V rows of layers 0 and 23 of one plain generate."""
    tok = eng.t2s_generate([u], sampler(greedy))[0].tolist()
    kv = [t.cpu().numpy() for layer in (0, 23) for t in eng.t2s_read_kv(layer)]
    return tok, kv


@pytest.fixture(scope="module")
def four(eng, sentences):
    """The present form (four stages), computed once: {(sentence, greedy): (tokens, K/V rows)}."""
    eng.set_vocoder_cus(0)
    eng.set_option("gemm_small_ns", 4)
    try:
        return {(i, g): _generate(eng, u, g) for i, u in enumerate(sentences) for g in (True, False)}
    finally:
        eng.set_option("gemm_small_ns", 0)


@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("i", [0, 1])
def test_forced_depths_are_bit_identical(eng, sentences, four, i, ns):
    eng.set_vocoder_cus(0)
    eng.set_option("gemm_small_ns", ns)
    try:
        for g in (True, False):
            tok, kv = _generate(eng, sentences[i], g)
            want_tok, want_kv = four[(i, g)]
            assert len(tok) > 0 and tok == want_tok, f"sentence {i} ns {ns} greedy {g}"
            for a, b in zip(kv, want_kv):
                assert a.shape == b.shape and a.shape[0] >= (36, 81)[i]
                assert np.array_equal(a, b), f"sentence {i} ns {ns} greedy {g}"
    finally:
        eng.set_option("gemm_small_ns", 0)


def test_option_is_validated(eng):
    from genie_tts_amd.engine import EngineError
    for bad in (1, 5, -1):
        with pytest.raises(EngineError):
            eng.set_option("gemm_small_ns", bad)


def run_stream(eng, utts, sp):
    """bench.py's Runner.stream call pattern: prefetch i+2, start i+1, finish i."""
    n = len(utts)
    if n > 1:
        eng.t2s_prefetch(utts[1], sp)
    eng.t2s_generate_start(utts[0], sp)
    got = []
    for i in range(n):
        if i + 1 < n:
            if i + 2 < n:
                eng.t2s_prefetch(utts[i + 2], sp)
            eng.t2s_generate_start(utts[i + 1], sp)
        got.append(eng.t2s_generate_finish().tolist())
    return got


@pytest.mark.parametrize("K", [64, 8])
@pytest.mark.parametrize("greedy", [True, False])
def test_stream_with_prefetches_matches_plain(eng, sentences, four, K, greedy):
    """The rule (option 0), prefetches on the K vocoder CUs.  At K = 8 every prefill grid of these
    sentences exceeds the stream's CUs, so the rule itself picks the two-stage form."""
    # four distinct tuple objects (a prefetch is matched to its generate by the tuple's identity)
    utts = [sentences[0], sentences[1], sentences[0][:5] + (STEPS,), sentences[1][:5] + (STEPS,)]
    want = [four[(0, greedy)][0], four[(1, greedy)][0]] * 2
    eng.set_option("gemm_small_ns", 0)
    if K == 8:
        eng.set_option("decode_cus", 224)   # the decode CUs are a multiple of 32: 224 of the 248 left
    try:
        eng.set_vocoder_cus(K)
        t0 = eng.counter("persist_timeouts")
        got = run_stream(eng, utts, sampler(greedy))
        assert got == want
        assert eng.counter("persist_timeouts") == t0
    finally:
        eng.set_vocoder_cus(0)
        eng.set_option("decode_cus", 0)
