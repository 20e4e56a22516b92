"""Cost of a fused reference set (timbre fusion), written to
profiles/timbre_mix_cost.json.  Every figure is a median over --runs runs (>= 3) with its min and
max beside it, a host clock around work that ends in a device synchronise.

  set      api.set_reference_features plus the first ReferenceAudio.cond for n = 1, 2, 4, 8 clips of
           5 s, fresh clips every run (nothing cached): n reference-encoder passes, on V2ProPlus
           also n passes of the SV model (api.load_sv_model, synthetic weights) and of the sv_emb
           GEMV, then one mix launch (and one projection on V2ProPlus).  n = 1 is today's path.
  weights  the same clips set again with other weights, then cond: nothing is encoded, one mix
           launch (two launches on V2ProPlus).
  lookup   a further cond on the same reference: the cached dictionary.
Synthetic characters, V2 and V2ProPlus.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECONDS = 5
COUNTS = (1, 2, 4, 8)


def _stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=len(v))


def measure(torch, version, runs):
    from genie_tts_amd import api, audio as A, synth
    from genie_tts_amd.model_manager import build_model, model_manager
    v2pp = version != "v2"
    m = build_model(synth.synthetic_character(version), version, vits_noise="zero")
    phones, ssl = synth.synth_phones(12, "tm-r"), synth.synth_ssl(41, "tm-s")

    def clips(n, tag):
        c = [synth.synth_ref_audio(SECONDS * 32000, f"tm-{tag}-{i}") for i in range(n)]
        return c, [A.resample(x[0], 32000, 16000).reshape(1, -1) for x in c] if v2pp else None

    def set_and_cond(c, c16, weights):
        """ms of set_reference_features + the SV embeddings + cond, device idle at both ends."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.set_reference_features("tm", phones, None, c[0], ssl, aux_audio_32k=c[1:] or None,
                                   aux_weights=weights if len(c) > 1 else None)
        ref = api._reference_audios["tm"]
        if v2pp:                      # the 16 kHz copies a clip read from a file carries
            ref.audio_16k, ref.aux_audio_16k = c16[0], list(c16[1:])
            api._ensure_sv_emb(m, ref)
        ref.cond(m.VITS, m.PROMPT_ENCODER)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ref

    out = {}
    try:
        for n in COUNTS:
            ts, tw, tl = [], [], []
            for run in range(runs + 1):          # run 0 warms every shape up and is dropped
                c, c16 = clips(n, f"{n}-{run}")
                api.clear_reference_audio_cache()
                t, ref = set_and_cond(c, c16, [1.0] * n)
                if n > 1:
                    sv = [ref.sv_emb, *ref.aux_sv_emb] if v2pp else None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    api.set_reference_features("tm", phones, None, c[0], ssl, sv_emb=sv[0] if v2pp else None,
                                               aux_audio_32k=c[1:], aux_sv_emb=sv[1:] if v2pp else None,
                                               aux_weights=[2.0] + [1.0] * (n - 1))
                    ref = api._reference_audios["tm"]
                    ref.cond(m.VITS, m.PROMPT_ENCODER)
                    torch.cuda.synchronize()
                    w = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                ref.cond(m.VITS, m.PROMPT_ENCODER)
                torch.cuda.synchronize()
                look = (time.perf_counter() - t0) * 1e3
                if run:
                    ts.append(t)
                    tl.append(look)
                    if n > 1:
                        tw.append(w)
            out[str(n)] = dict(set_ms=_stat(ts), lookup_ms=_stat(tl), **({"weights_ms": _stat(tw)} if n > 1 else {}))
            print(version, n, json.dumps(out[str(n)]), flush=True)
    finally:
        api.clear_reference_audio_cache()
        m.ENGINE.close()
        if v2pp:
            model_manager.unload_sv_model()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timbre_mix_cost.json"))
    a = ap.parse_args()
    assert a.runs >= 3
    import torch
    from genie_tts_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), clip_seconds=SECONDS, runs=a.runs)
    res["v2"] = measure(torch, "v2", a.runs)
    api.load_sv_model(synth.synth_sv_weights())
    res["v2ProPlus"] = measure(torch, "v2ProPlus", a.runs)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
