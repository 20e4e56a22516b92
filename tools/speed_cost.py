"""Cost of a speech-rate call: one utterance's VITS (G = 80, S = 45, V2, Philox noise) at
speeds 0.8 / 1.0 / 1.25 -- T', median time per call over `--iters` calls (HIP events around
Engine.vits_decode, the host's overflow-flag sync included), one JSON line per speed.
Under `rocprofv3 --kernel-trace --stats -- python tools/speed_cost.py` the stats hold
k_interp_linear's own time (two of the three speeds launch it, once per call).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--tokens", type=int, default=80)
    a = ap.parse_args()
    import torch
    from genie_tts_amd import synth
    from genie_tts_amd.engine import Engine
    w = synth.synthetic_character("v2")
    e = Engine({k: w[k] for k in ("t2s_encoder", "t2s", "vits")}, "v2")
    try:
        G = a.tokens
        txt = synth.synth_phones(45, "speed-cost")
        sem = ((np.arange(G, dtype=np.int64) * 37 + 11) % 1024).reshape(1, 1, G)
        ge = e.ref_encode(synth.synth_ref_audio(32000 * 2 + 1234))
        for speed in (0.8, 1.0, 1.25):
            for _ in range(3):
                e.vits_decode(txt, sem, ge=ge, noise_seed=7, speed=speed)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.iters):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                e.vits_decode(txt, sem, ge=ge, noise_seed=7, speed=speed)
                t1.record()
                t1.synchronize()
                ms.append(t0.elapsed_time(t1))
            frames = e.vits_frames(G, speed)
            print(json.dumps(dict(speed=speed, n_sem=G, frames=frames, samples=640 * frames, iters=a.iters,
                                  vits_ms_median=float(np.median(ms)), vits_ms_min=float(np.min(ms)),
                                  ms_per_frame=float(np.median(ms)) / frames)), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
