"""Cost of the sentence join on the GPU (edge-silence trim and pause), written to
profiles/join_bench.json.  Every figure is a median over --runs runs (>= 3) with its min and max
beside it.

  stage     one 3.2 s item (102400 samples at 32 kHz, speech between two silences) to 48 kHz int16,
            HIP events around the call:
              convert    gsv_audio_convert: the output stage alone, as the parent commit has it;
              join       gsv_audio_join with pause=0.3, trim=-50: the frame pass, the span pass, then
                         the stage over the span and the pause (call times, not kernel times);
              pause      gsv_audio_join with pause=0.3 alone: the span pass and the stage.
  stream    the configs[1] sentence stream of bench.py (--steps sentences, vocoder on 64 CUs), each
            sentence delivered to the host as 48 kHz int16 bytes:
              gpu    sample_rate=48000, pcm16=True, pause=0.3, trim=-50 on the vocoder item;
              plain  the same stream without the two options (the parent commit's path);
              host   what a caller needs without them: the float32 audio copied to the host, the
                     oracle's scan (tests/trim_oracle.py), the cut and the pad, then audio.resample
                     and audio.to_pcm16.
            The three alternate within a run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAUSE, TRIM = 0.3, -50.0


def _stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=len(v))


def _event_ms(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stage(torch, eng, runs, iters):
    import ctypes
    from genie_tts_amd.engine import Join, _stream, join_samples, lib
    n = 1280 * 80
    x = torch.zeros(n, device=eng.dev)
    x[n // 8: n - n // 8] = (torch.rand(n - 2 * (n // 8), device=eng.dev) * 2 - 1) * 0.3
    out = torch.empty(join_samples(n, 48000, PAUSE), dtype=torch.int16, device=eng.dev)
    span = torch.zeros(4, dtype=torch.int32, device=eng.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def join(trim):   # the C entry itself: the Python binding would add the span's copy to the host
        j = Join(0.0, 0.0, None, trim, PAUSE, span.data_ptr())
        return lambda: lib().gsv_audio_join(eng.h, p(x), n, ctypes.byref(j), 48000, 1, p(out), _stream())
    forms = dict(convert=lambda: lib().gsv_audio_convert(eng.h, p(x), n, 48000, 1, p(out), _stream()),
                 join=join(TRIM), pause=join(0.0))
    res = {}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        meds = [float(np.median([_event_ms(torch, fn) for _ in range(iters)])) * 1e3 for _ in range(runs)]
        res[name] = dict(call_us=_stat(meds))
    forms["join"]()
    res["n_in"] = n
    res["span"] = [int(v) for v in span.cpu()]
    return res


def host_join(x):
    """What a caller does on the host with the float32 audio of a sentence."""
    from genie_tts_amd import audio as A
    from tests import trim_oracle as O
    y = A.resample(O.join(x, PAUSE, TRIM), 32000, 48000)
    return A.to_pcm16(y)


def stream_once(run, n, mode):
    """bench.Runner.stream with each sentence delivered to the host as `mode` says; -> bytes out."""
    eng = run.eng
    utts = [(run.d_ref, t, run.d_ref_bert, run.d_bert[0], run.d_ssl, run.items[0].force_steps)
            for t in (run.d_txt[0], run.d_txt[0].clone())]
    utt = lambda i: utts[i % 2]
    cond = dict(ge=run.ge_v2)
    fmt = dict(gpu=dict(sample_rate=48000, pcm16=True, pause=PAUSE, trim=TRIM),
               plain=dict(sample_rate=48000, pcm16=True), host={})[mode]
    nbytes = 0

    def deliver(t):
        if mode == "host":
            return len(host_join(t.cpu().numpy()))
        return len(eng.vits_joined([t])[0].cpu().numpy().tobytes())
    eng.t2s_prefetch(utt(1), run.sp)
    eng.t2s_generate_start(utt(0), run.sp)
    pending = None
    for i in range(n):
        if i + 1 < n:
            if i + 2 < n:
                eng.t2s_prefetch(utt(i + 2), run.sp)
            eng.t2s_generate_start(utt(i + 1), run.sp)
        sem = eng.t2s_generate_finish()
        if pending is not None:
            eng.vits_wait()
            nbytes += deliver(pending)
        pending = eng.vits_decode_async(dict(text_seq=utt(i)[1], pred_semantic=sem, noise_seed=run.seed, **cond, **fmt))
    eng.vits_wait()
    nbytes += deliver(pending)
    return nbytes


def stream(torch, run, runs, steps):
    eng = run.eng
    eng.set_vocoder_cus(64)
    try:
        modes = ("plain", "gpu", "host")
        for m in modes:
            stream_once(run, 4, m)
        torch.cuda.synchronize()
        ms = {m: [] for m in modes}
        for r in range(runs):
            for m in modes[r % 3:] + modes[:r % 3]:   # alternate, rotating the order
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stream_once(run, steps, m)
                torch.cuda.synchronize()
                ms[m].append((time.perf_counter() - t0) * 1e3 / steps)
        return {m: dict(ms_per_utterance=_stat(v)) for m, v in ms.items()} | dict(steps=steps)
    finally:
        eng.set_vocoder_cus(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="stage: calls per run")
    ap.add_argument("--steps", type=int, default=100, help="stream: sentences per run")
    ap.add_argument("--only", choices=("stage", "stream"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_bench.json"))
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs: at least 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("join_bench needs a GPU: there is no CPU path to time")
    import bench
    from genie_tts_amd import workloads
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "pause_s": PAUSE, "trim_dbfs": TRIM}
    wl = workloads.single()
    run = bench.Runner(wl, wl.items, dev, 0)
    try:
        if a.only in (None, "stage"):
            res["stage"] = stage(torch, run.eng, a.runs, a.iters)
        if a.only in (None, "stream"):
            res["stream"] = stream(torch, run, a.runs, a.steps)
    finally:
        run.eng.close()
    print(json.dumps(res), flush=True)
    if a.only is None:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
