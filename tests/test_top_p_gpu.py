"""GPU: nucleus sampling (gsv_sampler.top_p) -- the sampler body against the float64-cut
oracle (tests/top_p_oracle.py) through debug_sample, and the decode paths that share it
(per-step graphs, the session calls, the three persistent kernels) against each other.

Every oracle case asserts margin >= 1e-4 on its own rows (an assertion on the inputs: a
float32 cumulative sum may legitimately differ from the float64 one below that), with
top_p chosen by pick_top_p.  Inputs are built by the module-level functions below so the
host tests can check the same margins without a GPU.
"""
import math

import numpy as np
import pytest

from tests import top_p_oracle as O
from tests.philox import sampler_noise

pytestmark = pytest.mark.gpu
SEED = 0x1234_5678_9ABC
B = 4


# ------------------------------------------------------------------ inputs (CPU)
def _hists(rng, sizes, avoid=()):
    pool = np.setdiff1d(np.arange(1025), np.asarray(avoid, np.int64))
    return [rng.choice(pool, size=n, replace=False) for n in sizes]


def random_rows(seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 5, size=(B, 1025)).astype(np.float32)
    return logits, _hists(rng, (0, 37, 121, 200))


def plateau_rows(seed=7):
    """400 entries 6 + N(0, 0.3), the rest -6 + N(0, 1): hundreds of survivors."""
    rng = np.random.default_rng(seed)
    logits = (-6 + rng.normal(0, 1, size=(B, 1025))).astype(np.float32)
    for b in range(B):
        idx = rng.choice(1025, size=400, replace=False)
        logits[b, idx] = (6 + rng.normal(0, 0.3, size=400)).astype(np.float32)
    return logits, _hists(rng, (0, 10, 60, 200))


def tie_rows(seed=11):
    """10 distinct leaders, then 30 exactly equal entries that straddle the cut."""
    rng = np.random.default_rng(seed)
    logits = (-8 + rng.normal(0, 1, size=(B, 1025))).astype(np.float32)
    tied = []
    for b in range(B):
        idx = rng.choice(1025, size=40, replace=False)
        logits[b, idx[:10]] = np.linspace(5.0, 4.1, 10).astype(np.float32)
        logits[b, idx[10:]] = np.float32(3.0)
        tied.append(np.sort(idx[10:]))
    hists = [rng.choice(np.setdiff1d(np.arange(1025), tied[b]), size=n, replace=False)
             for b, n in enumerate((0, 5, 20, 50))]
    return logits, hists, tied


def tie_top_p(logits, hists):
    """The midpoint between the cumulative sums at two neighbouring tied entries (the 15th and
    16th of row 0's), moved by pick_top_p's grid only if another row asks for it."""
    _, S = O.cum_probs(O.penalised(logits[0], hists[0]))
    return float(np.float32(0.5 * (float(S[24]) + float(S[25]))))


def few_rows(seed=13):
    """Rows led by 1-3 heavy tokens: fewer survivors than top_k."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 1, size=(B, 1025)).astype(np.float32)
    lead = [(12.0,), (9.0, 8.2), (9.0, 8.6, 8.0), (8.0, 7.9, 7.8, 7.7)]
    pos = []
    for b in range(B):
        idx = rng.choice(np.arange(1, 1025), size=len(lead[b]), replace=False)
        logits[b, idx] = np.asarray(lead[b], np.float32)
        pos.append(idx)
    return logits, [np.zeros(0, np.int64)] * B, pos


def sole_survivor_step(index, b, lo=1, hi=200):
    """A step whose Philox normal at (index, step, b) is negative."""
    for step in range(lo, hi):
        if sampler_noise(1025, step, b, SEED)[index] < 0:
            return step
    raise AssertionError("no negative q found")


# ------------------------------------------------------------------ helpers (GPU)
def _run(logits, hists, sp, step):
    import torch
    from genie_tts_amd.engine import debug_sample
    seen = np.stack([O.seen_bits(h) for h in hists])
    tok, stop = debug_sample(torch.from_numpy(np.ascontiguousarray(logits)).cuda(), torch.from_numpy(seen).cuda(),
                             sp, step)
    return tok.cpu().numpy(), stop.cpu().numpy()


def _check(logits, hists, top_p, top_k, temp, step, greedy=False):
    from genie_tts_amd.engine import make_sampler
    for b in range(len(hists)):
        m = O.margin(logits[b], hists[b], top_p)
        print(f"row {b}: top_p {top_p:.6f} margin {m:.3e} survivors "
              f"{int(O.survivors(O.penalised(logits[b], hists[b]), top_p).sum())}")
        assert m >= O.MARGIN, (b, m)
    sp = make_sampler(top_k=top_k, temperature=temp, greedy=greedy, seed=SEED, top_p=top_p)
    tok, stop = _run(logits, hists, sp, step)
    for b in range(len(hists)):
        q = np.ones(1025, np.float32) if greedy else sampler_noise(1025, step, b, SEED)
        t_ref, raw = O.sample(logits[b], hists[b], q, top_k, temp, top_p=top_p)
        assert int(tok[b]) == t_ref, (b, int(tok[b]), t_ref)
        assert bool(stop[b]) == (raw == 1024 or t_ref == 1024)


# ------------------------------------------------------------------ the sampler body
@pytest.mark.parametrize("target", [0.5, 0.9, 0.99])
@pytest.mark.parametrize("top_k,temp", [(15, 0.7), (15, 1.0), (64, 0.7), (64, 1.0)])
def test_random_rows_match_oracle(target, top_k, temp):
    logits, hists = random_rows(int(target * 100) * 1000 + top_k * 10 + int(temp * 10))
    top_p = O.pick_top_p(list(zip(logits, hists)), target)
    _check(logits, hists, top_p, top_k, temp, step=13)


def test_many_survivors():
    """The cut lies hundreds of ranks deep: an implementation that sorts only a few leaders, or
    only the top-k candidates, gets it wrong."""
    logits, hists = plateau_rows()
    top_p = O.pick_top_p(list(zip(logits, hists)), 0.6)
    n = [int(O.survivors(O.penalised(l, h), top_p).sum()) for l, h in zip(logits, hists)]
    assert all(150 <= k <= 350 for k in n), n
    _check(logits, hists, top_p, 64, 1.0, step=5)


@pytest.mark.parametrize("step", [1, 2, 3, 5, 8, 13, 21, 34])
def test_tie_at_the_cut_keeps_the_lowest_indices(step):
    logits, hists, tied = tie_rows()
    top_p = tie_top_p(logits, hists)
    keep = O.survivors(O.penalised(logits[0], hists[0]), top_p).numpy()
    kept = [int(i) for i in tied[0] if keep[i]]
    assert 0 < len(kept) < 30 and kept == tied[0][:len(kept)].tolist()   # the lowest tied indices
    _check(logits[:1].repeat(B, 0), [hists[0]] * B, top_p, 64, 1.0, step)


def test_tied_survivors_vary_over_the_steps():
    """The eight steps above do not all pick the same token (so the tie test sees who survived)."""
    logits, hists, _ = tie_rows()
    top_p = tie_top_p(logits, hists)
    toks = {O.sample(logits[0], hists[0], sampler_noise(1025, s, 0, SEED), 64, 1.0, top_p=top_p)[0]
            for s in (1, 2, 3, 5, 8, 13, 21, 34)}
    assert len(toks) >= 3


def test_fewer_survivors_than_top_k():
    logits, hists, pos = few_rows()
    top_p = O.pick_top_p(list(zip(logits, hists)), 0.75)
    n = [int(O.survivors(O.penalised(l, h), top_p).sum()) for l, h in zip(logits, hists)]
    assert all(1 <= k <= 3 for k in n) and n[0] == 1, n
    step = sole_survivor_step(int(pos[0][0]), 0)          # row 0: its only survivor meets q < 0
    assert sampler_noise(1025, step, 0, SEED)[int(pos[0][0])] < 0
    _check(logits, hists, top_p, 15, 1.0, step)
    t_ref, _ = O.sample(logits[0], hists[0], sampler_noise(1025, step, 0, SEED), 15, 1.0, top_p=top_p)
    assert t_ref != int(pos[0][0])                        # argmax(p / q) over the zeros, not the survivor


@pytest.mark.parametrize("top_p", [1.0, 0.0])
def test_top_p_one_and_unset_are_todays_sampler(top_p):
    """tests/test_sampler_gpu.py's inputs: top_p 1 and a zero field equal oracle.restate.sample."""
    from genie_tts_amd.engine import make_sampler
    top_k, temp, step, Bs = 15, 1.0, 13, 7
    rng = np.random.default_rng(top_k * 100 + int(temp * 10) + 0)
    logits = rng.normal(0, 3, size=(Bs, 1025)).astype(np.float32)
    logits[2, :40] = logits[2].max() + 1.0
    logits[3, 100:130] = 2.5
    logits[3, 500:505] = 9.0
    logits[4, 1024] = logits[4].max() + 5.0
    hists = [rng.choice(1025, size=int(rng.integers(0, 200)), replace=False) for _ in range(Bs)]
    sp = make_sampler(top_k=top_k, temperature=temp, greedy=False, seed=SEED)
    sp.top_p = top_p
    tok, stop = _run(logits, hists, sp, step)
    for b in range(Bs):
        t_ref, raw = O.restate_sample(logits[b], hists[b], sampler_noise(1025, step, b, SEED), top_k, temp)
        assert int(tok[b]) == t_ref, b
        assert bool(stop[b]) == (raw == 1024 or t_ref == 1024)


def test_greedy_ignores_top_p():
    from genie_tts_amd.engine import make_sampler
    logits, hists = random_rows(3)
    a, _ = _run(logits, hists, make_sampler(greedy=True, top_p=0.3), 4)
    b, _ = _run(logits, hists, make_sampler(greedy=True, top_p=1.0), 4)
    assert a.tolist() == b.tolist()


def test_non_finite_logits_return():
    """NaN and +inf entries under top_p: the call returns (every loop is bounded), and the
    sampler is sound afterwards."""
    from genie_tts_amd.engine import make_sampler
    logits, hists = random_rows(5)
    bad = logits.copy()
    bad[1, 10:20] = np.nan
    bad[1, 500] = np.inf
    bad[2, 7] = np.inf
    tok, _ = _run(bad, hists, make_sampler(greedy=False, seed=SEED, top_p=0.8), 3)
    assert tok.shape == (B,) and all(0 <= int(t) <= 1024 for t in tok)
    top_p = O.pick_top_p(list(zip(logits, hists)), 0.8)
    _check(logits, hists, top_p, 15, 1.0, step=3)


# ------------------------------------------------------------------ the decode paths
@pytest.fixture(scope="module")
def eng():
    from genie_tts_amd.engine import Engine
    from tests.common import character
    w = character("v2")
    e = Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")
    yield e
    e.close()


def _fresh():
    from genie_tts_amd.engine import Engine
    from tests.common import character
    w = character("v2")
    return Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")


@pytest.fixture(scope="module")
def tight(eng):
    """A top_p that bites on the synthetic model, whose logits are nearly flat (p ~ 1 / 1025
    each, so 0.8 or 0.3 keep hundreds of tokens and the top-k of 15 hides them): the midpoint
    between the 4th and 5th cumulative probability of one first-stage logits row -- about four
    survivors per step, fewer than top_k."""
    import torch
    from tests.common import t2s_inputs
    ref, txt, rb, tb, ssl = t2s_inputs(R=12, S=10, H=41, tag="tp1")
    x, prompts = eng.t2s_encode(ref, txt, None, None, ssl)
    _, logits = eng.t2s_prefill(x, prompts)
    _, S = O.cum_probs(torch.as_tensor(logits.cpu().numpy()))
    p = float(np.float32(0.5 * (float(S[3]) + float(S[4]))))
    print(f"tight top_p {p:.6f} (S[0] {float(S[0]):.6f}, tokens to 0.3: {int((S <= 0.3).sum())})")
    return p


@pytest.fixture(params=["0.8", "tight"])
def top_p(request, tight):
    return 0.8 if request.param == "0.8" else tight


def _sp(top_p, steps=12, seed=1234, top_k=15):
    from genie_tts_amd.engine import make_sampler
    return make_sampler(top_k=top_k, greedy=False, seed=seed, force_steps=steps, top_p=top_p)


def _gen(eng, inps, sp, persist):
    eng.set_option("persist", persist)
    try:
        return [t.tolist() for t in eng.t2s_generate(inps, sp)]
    finally:
        eng.set_option("persist", 1)


@pytest.mark.parametrize("bad", [-0.1, 1.5, math.nan])
def test_bad_top_p_is_an_error_at_every_entry_point(eng, bad):
    import torch
    from genie_tts_amd.engine import EngineError, debug_sample, make_sampler
    from tests.common import t2s_inputs
    sp = make_sampler(greedy=False, force_steps=4)
    sp.top_p = bad
    inp = t2s_inputs(R=10, S=8, H=30, tag="tpbad")
    with pytest.raises(EngineError, match="top_p"):
        debug_sample(torch.zeros((1, 1025), device="cuda"), torch.zeros((1, 33), dtype=torch.int32, device="cuda"),
                     sp, 1)
    with pytest.raises(EngineError, match="top_p"):
        eng.t2s_generate([inp], sp)
    with pytest.raises(EngineError, match="top_p"):
        eng.t2s_prefill(np.zeros((18, 512), np.float32), np.zeros(15, np.int64), sp)
    with pytest.raises(EngineError, match="top_p"):
        eng.t2s_generate_start(inp, sp)
    assert eng.t2s_generate([inp], make_sampler(force_steps=4))[0].size > 0      # the engine is fine


def test_single_sequence_paths_agree(eng, top_p):
    """k_decode_persist1 == per-step graphs == t2s_prefill + t2s_decode_steps under top_p."""
    from oracle import restate as R
    from tests.common import t2s_inputs
    inp = t2s_inputs(R=12, S=10, H=41, tag="tp1")
    steps = 12
    sp = _sp(top_p, steps)
    a = _gen(eng, [inp], sp, 1)[0]
    b = _gen(eng, [inp], sp, 0)[0]
    assert a == b and len(a) == steps - 1
    ref, txt, rb, tb, ssl = inp
    x, prompts = eng.t2s_encode(ref, txt, None, None, ssl)
    eng.t2s_prefill(x, prompts, sp)
    y, _, _ = eng.t2s_decode_steps(steps, sp)
    n = int(prompts.numel()) + 1 + steps
    sess = R.trim_tokens(y[:n].cpu().numpy().tolist(), steps - 1).reshape(-1).tolist()
    assert sess[:-1] == a[:-1] and len(sess) == len(a)


def test_multi_sequence_kernel_agrees(eng, top_p):
    """B = 3 on k_decode_persist1m == graphs, and the sentence in slot 0 == its own B = 1
    generate.  (The sampler's Philox counter holds the batch slot, so a sampled sentence in
    slot i > 0 draws other noise than alone in slot 0, with or without top_p; batched and
    single runs of those are compared in greedy mode only, as tests/test_persist_gpu.py does.)"""
    from tests.common import t2s_inputs
    inps = [t2s_inputs(R=10 + 2 * i, S=8 + i, H=30 + 4 * i, tag=f"tpm{i}") for i in range(3)]
    sp = _sp(top_p)
    a = _gen(eng, inps, sp, 1)
    assert a == _gen(eng, inps, sp, 0)
    assert _gen(eng, inps[:1], sp, 1)[0] == a[0]
    for order in ([1, 0, 2], [2, 1, 0]):          # every sentence once in slot 0: equal to its own generate
        got = _gen(eng, [inps[i] for i in order], sp, 1)
        assert got[0] == _gen(eng, [inps[order[0]]], sp, 1)[0], order


def test_batched_mfma_kernel_agrees(eng, top_p):
    """k_decode_persistm (persistm_min_b lowered to 2) == graphs."""
    from tests.common import t2s_inputs
    inps = [t2s_inputs(R=10 + 3 * i, S=8 + 2 * i, H=30 + 6 * i, tag=f"tpmm{i}") for i in range(3)]
    sp = _sp(top_p)
    eng.set_option("persistm", 1)
    eng.set_option("persistm_min_b", 2)
    try:
        a = _gen(eng, inps, sp, 1)
    finally:
        eng.set_option("persistm_min_b", 32)
    assert a == _gen(eng, inps, sp, 0)


def test_step_graph_is_keyed_by_top_p(eng, tight):
    """A step graph captured under one top_p must not replay for another: top_p 1, then 0.5
    and the biting value, then 1 again on one engine; each equals a fresh engine's run."""
    from tests.common import t2s_inputs
    inp = t2s_inputs(R=12, S=10, H=41, tag="tpk")
    steps = 40
    first = _gen(eng, [inp], _sp(1.0, steps), 0)[0]
    second = _gen(eng, [inp], _sp(0.5, steps), 0)[0]
    bites = _gen(eng, [inp], _sp(tight, steps), 0)[0]
    third = _gen(eng, [inp], _sp(1.0, steps), 0)[0]
    assert first == third and bites != first
    e2 = _fresh()
    try:
        assert bites == _gen(e2, [inp], _sp(tight, steps), 0)[0]
        assert second == _gen(e2, [inp], _sp(0.5, steps), 0)[0]
    finally:
        e2.close()


@pytest.mark.parametrize("which", ["0.5", "tight"])
def test_prefetch_under_another_top_p_is_not_reused(eng, tight, which):
    from tests.common import t2s_inputs
    p = 0.5 if which == "0.5" else tight
    inp = t2s_inputs(R=12, S=10, H=41, tag="tpf")
    plain = _gen(eng, [inp], _sp(p), 1)[0]
    eng.set_vocoder_cus(64)
    try:
        eng.t2s_prefetch(inp, _sp(1.0))
        got = eng.t2s_generate([inp], _sp(p))[0].tolist()
    finally:
        eng.set_vocoder_cus(0)
    assert got == plain


def test_top_p_changes_the_tokens(eng, tight):
    """One seed, 48 forced steps: a nucleus tighter than top_k and none differ, on every path.
    (At 0.3 the synthetic model's near-flat distribution keeps ~300 tokens, more than top_k,
    and the run equals the one without top_p: measured, so the generate paths use `tight`
    and the sampler body is shown at 0.3 on the N(0, 5) rows below.)"""
    from tests.common import t2s_inputs
    inp = t2s_inputs(R=12, S=10, H=41, tag="tpd")
    b = _gen(eng, [inp], _sp(1.0, 48, seed=99), 1)[0]
    for persist in (1, 0):
        a = _gen(eng, [inp], _sp(tight, 48, seed=99), persist)[0]
        assert len(a) == len(b) == 47 and a != b, persist
    inps = [t2s_inputs(R=10 + 2 * i, S=8 + i, H=30 + 4 * i, tag=f"tpm{i}") for i in range(3)]
    assert _gen(eng, inps, _sp(tight, 48, seed=99), 1) != _gen(eng, inps, _sp(1.0, 48, seed=99), 1)


def test_top_p_changes_the_sampler_at_0_3():
    from genie_tts_amd.engine import make_sampler
    logits, hists = random_rows(50157)
    top_p = O.pick_top_p(list(zip(logits, hists)), 0.3)
    differ = 0
    for step in range(1, 11):
        a, _ = _run(logits, hists, make_sampler(greedy=False, seed=SEED, top_p=top_p), step)
        b, _ = _run(logits, hists, make_sampler(greedy=False, seed=SEED, top_p=1.0), step)
        differ += int((a != b).sum())
    assert differ >= 1


# ------------------------------------------------------------------ the API
def test_api_keywords_equal_an_explicit_sampler():
    import asyncio
    import genie_tts_amd as G
    from genie_tts_amd import api, synth
    from genie_tts_amd.engine import make_sampler
    from genie_tts_amd.model_manager import build_model, model_manager
    from tests.common import character
    own = make_sampler(greedy=False, seed=5, max_steps=16)
    m = build_model(character("v2"), "v2", sampler=own)
    m.VITS.noise = "zero"
    name = "top-p-char"
    try:
        model_manager._put(name, m)
        model_manager.character_to_language[name] = "Japanese"
        txt = synth.synth_phones(10, "tp-t")
        G.set_reference_features(name, synth.synth_phones(12, "tp-r"), None, synth.synth_ref_audio(64000, "tp-a"),
                                 synth.synth_ssl(41, "tp-s"))
        explicit = make_sampler(greedy=False, seed=77, max_steps=16, top_p=0.6)
        want = G.tts(name, txt, split_sentence=False, sampler=explicit)
        got = G.tts(name, txt, split_sentence=False, top_p=0.6, seed=77)
        np.testing.assert_array_equal(got, want)

        async def go(**kw):
            return [c async for c in api.tts_async(name, txt, **kw)]
        assert asyncio.run(go(top_p=0.6, seed=77)) == asyncio.run(go(sampler=explicit))
        assert asyncio.run(go(top_p=0.6, seed=77)) == [api.A.to_pcm16(want)]
        plain = G.tts(name, txt, split_sentence=False)
        np.testing.assert_array_equal(plain, G.tts(name, txt, split_sentence=False, sampler=own))
        assert asyncio.run(go()) == [api.A.to_pcm16(plain)]
    finally:
        model_manager.character_to_model.pop(name, None)
        api.clear_reference_audio_cache()
        m.ENGINE.close()
