"""Cost of nucleus sampling in the persistent decode: the persistent launch's time
(gsv_get_kernel_timing) of sampled generates with top_p = 1 against top_p = 0.8, alternating,
for (a) one sentence at 81 forced steps (k_decode_persist1) and (b) the batch64 workload's
generate (k_decode_persistm).  One JSON line per case: median launch time under each setting
and the difference per decode step.  top_p = 1 runs exactly the code of a sampler without
the field, so its figure is the reference.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launch_us(eng, utts, sp):
    eng.set_timing(True)                      # resets the launch-time accumulator
    eng.t2s_generate(utts, sp)
    us, n = eng.kernel_timing()
    if n <= 0:
        raise RuntimeError(f"no persistent launch was timed ({n})")
    return us * n                             # all launches of the generate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--top-p", type=float, default=0.8)
    a = ap.parse_args()
    from genie_tts_amd import synth, workloads
    from genie_tts_amd.engine import Engine, make_sampler
    w = synth.synthetic_character("v2")
    e = Engine({k: w[k] for k in ("t2s_encoder", "t2s")}, "v2")
    try:
        e.set_option("persist", 1)
        one, b64 = workloads.single(), workloads.batch64()
        cases = [("B=1, 81 steps", one, 15, 81), ("batch64 generate", b64, b64.top_k, 0)]
        for name, wl, top_k, force in cases:
            r = wl.reference
            utts = [tuple(e._dev(x, None) for x in (r.ref_seq, it.text_seq, r.ref_bert,
                                                    np.zeros((it.text_seq.shape[-1], 1024), np.float32), r.ssl))
                    + (force or it.force_steps,) for it in wl.items]
            steps = max(u[-1] for u in utts)
            sps = {p: make_sampler(top_k=top_k, greedy=False, seed=1234, top_p=p) for p in (1.0, a.top_p)}
            for sp in sps.values():
                for _ in range(2):
                    launch_us(e, utts, sp)
            us = {p: [] for p in sps}
            for _ in range(a.iters):
                for p, sp in sps.items():
                    us[p].append(launch_us(e, utts, sp))
            med = {p: float(np.median(v)) for p, v in us.items()}
            print(json.dumps(dict(case=name, B=len(utts), steps=steps, iters=a.iters, top_p=a.top_p,
                                  launch_us_top_p_1=med[1.0], launch_us_top_p=med[a.top_p],
                                  spread_us_top_p_1=float(np.max(us[1.0]) - np.min(us[1.0])),
                                  per_step_us=(med[a.top_p] - med[1.0]) / steps,
                                  per_step_us_base=med[1.0] / steps)), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
