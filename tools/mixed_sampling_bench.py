"""What one sampler per sequence buys a server whose requests carry sampling controls: the
batch64 workload's 64 ragged sentences (forced lengths) on the synthetic character with eight
distinct samplers, eight sentences each.

  A  one samplers= generate of 64 (gsv_t2s_generate_each)
  B  eight plain generates of 8, one per sampler -- what per-sampler rounds do

Host clock around the calls (a generate returns after its device synchronise), A and B
alternating; one JSON line with both medians, their spreads and the ratio.  The streams of A
are each sentence's position in its group of 8, so A draws B's noise; tokens_equal reports
whether the tokens came out equal too (the 64-wide and the 8-wide launch run different
kernels, whose logits may differ in the last bits).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from genie_tts_amd import synth, workloads
    from genie_tts_amd.engine import Engine, make_sampler
    w = synth.synthetic_character("v2")
    e = Engine({k: w[k] for k in ("t2s_encoder", "t2s")}, "v2")
    try:
        wl = workloads.batch64()
        r = wl.reference
        utts = [tuple(e._dev(x, None) for x in (r.ref_seq, it.text_seq, r.ref_bert,
                                                np.zeros((it.text_seq.shape[-1], 1024), np.float32), r.ssl))
                + (it.force_steps,) for it in wl.items]
        kinds = [dict(top_k=5), dict(top_k=15), dict(top_k=15, top_p=0.8), dict(top_k=5, temperature=0.8),
                 dict(top_k=30, top_p=0.9, temperature=1.2), dict(top_k=15, repetition_penalty=1.2),
                 dict(top_k=64), dict(top_k=10, top_p=0.95)]
        sps = [make_sampler(greedy=False, seed=1000 + i, **kw) for i, kw in enumerate(kinds)]
        each = [sps[i // 8] for i in range(64)]
        streams = [i % 8 for i in range(64)]

        def case_a():
            return e.t2s_generate(utts, samplers=each, streams=streams)

        def case_b():
            out = []
            for g in range(8):
                out += e.t2s_generate(utts[8 * g:8 * g + 8], sps[g])
            return out
        for _ in range(2):
            ta, tb = case_a(), case_b()
        same = all(x.tolist() == y.tolist() for x, y in zip(ta, tb))
        ms = {"A": [], "B": []}
        for _ in range(a.iters):
            for name, fn in (("A", case_a), ("B", case_b)):
                t0 = time.perf_counter()
                fn()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps(dict(workload=wl.name, sentences=64, samplers=8, iters=a.iters, tokens=wl.total_tokens,
                              one_generate_of_64_ms=med["A"], eight_generates_of_8_ms=med["B"],
                              spread_ms_A=float(np.max(ms["A"]) - np.min(ms["A"])),
                              spread_ms_B=float(np.max(ms["B"]) - np.min(ms["B"])),
                              ratio_B_over_A=med["B"] / med["A"], tokens_equal=same)), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
