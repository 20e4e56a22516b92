"""Cost of the output stage (sample rate + 16-bit PCM on the GPU), written to
profiles/sample_rate_bench.json.  Every figure is a median over --runs runs (>= 3) with its
min and max beside it.

  stage     per rate: one gsv_audio_convert call on the bench utterance's audio (G = 80, 102400
            samples), float32 and int16, HIP events around the call (the item-table copy + the
            kernel; a call time, not a kernel time).
  batch64   the 64 utterances of configs[2] through Engine.vits_decode_batch with rates cycling
            over all seven as int16 (one stage launch for the batch) and without the fields:
            two call times whose difference holds the stage.  `--only batch64-stage` runs just
            the former, for `rocprofv3 --kernel-trace --stats -- python tools/sample_rate_bench.py
            --only batch64-stage`, whose k_audio_out row is the 64-item launch's kernel time.
  stream    the configs[1] sentence stream of bench.py (--steps sentences, vocoder on 64 CUs),
            each sentence delivered to the host as 48 kHz int16 bytes:
              gpu    sample_rate=48000, pcm16=True on the vocoder item, then one device-to-host copy;
              host   what a caller must do without the stage: the default item, a device-to-host
                     copy of the float32 audio, audio.resample(32000 -> 48000) + audio.to_pcm16;
              plain  the default stream untouched (float32 left on the device, as bench.py times it):
                     the figure to hold against the parent commit's, with this session's spread.
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
    from genie_tts_amd.engine import SAMPLE_RATES, audio_samples
    x = torch.rand(1280 * 80, device=eng.dev) * 2 - 1
    out = {}
    for rate in SAMPLE_RATES:
        for pcm in (False, True):
            for _ in range(3):
                eng.audio_convert(x, rate, pcm16=pcm)
            torch.cuda.synchronize()
            meds = [float(np.median([_event_ms(torch, lambda: eng.audio_convert(x, rate, pcm16=pcm))
                                     for _ in range(iters)])) * 1e3 for _ in range(runs)]
            out[f"{rate}_{'int16' if pcm else 'float32'}"] = dict(call_us=_stat(meds), n_in=x.numel(),
                                                                  n_out=audio_samples(x.numel(), rate))
    return out


def batch64(torch, run, runs, only_stage=False):
    from genie_tts_amd.engine import SAMPLE_RATES
    eng = run.eng
    utts = [(run.d_ref, t, run.d_ref_bert, b, run.d_ssl, it.force_steps)
            for t, b, it in zip(run.d_txt, run.berts(0, len(run.items)), run.items)]
    sems = eng.t2s_generate(utts, run.sp)
    cond = dict(ge=run.ge_v2)
    plain = [dict(text_seq=t, pred_semantic=s, noise_seed=7 + i, **cond) for i, (t, s) in enumerate(zip(run.d_txt, sems))]
    rated = [dict(it, sample_rate=SAMPLE_RATES[i % len(SAMPLE_RATES)], pcm16=True) for i, it in enumerate(plain)]
    res = {}
    for name, items in (("with_stage", rated), ("without", plain)):
        if only_stage and name == "without":
            continue
        eng.vits_decode_batch(items)
        torch.cuda.synchronize()
        res[name] = dict(call_ms=_stat([_event_ms(torch, lambda: eng.vits_decode_batch(items)) for _ in range(runs)]))
    res["items"] = len(plain)
    res["samples_32k"] = int(sum(1280 * int(s.size) for s in sems))
    return res


def stream_once(run, n, mode):
    """bench.Runner.stream with each sentence delivered to the host as `mode` says; -> bytes out."""
    from genie_tts_amd import audio as A
    eng = run.eng
    utts = [(run.d_ref, t, run.d_ref_bert, run.d_bert[0], run.d_ssl, run.items[0].force_steps)
            for t in (run.d_txt[0], run.d_txt[0].clone())]
    utt = lambda i: utts[i % 2]
    cond = dict(ge=run.ge_v2)
    fmt = dict(sample_rate=48000, pcm16=True) if mode == "gpu" else {}
    nbytes = 0

    def deliver(t):
        if mode == "gpu":
            return len(t.cpu().numpy().tobytes())
        if mode == "host":
            return len(A.to_pcm16(A.resample(t.cpu().numpy(), 32000, 48000)))
        return 0
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
    ap.add_argument("--only", choices=("stage", "batch64", "batch64-stage", "stream"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rate_bench.json"))
    a = ap.parse_args()
    if a.runs < 3:
        ap.error("--runs: at least 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sample_rate_bench needs a GPU: there is no CPU path to time")
    import bench
    from genie_tts_amd import workloads
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs}
    if a.only in (None, "stage", "stream"):
        wl = workloads.single()
        run = bench.Runner(wl, wl.items, dev, 0)
        try:
            if a.only in (None, "stage"):
                res["stage"] = stage(torch, run.eng, a.runs, a.iters)
            if a.only in (None, "stream"):
                res["stream"] = stream(torch, run, a.runs, a.steps)
        finally:
            run.eng.close()
    if a.only in (None, "batch64", "batch64-stage"):
        wl = workloads.batch64()
        run = bench.Runner(wl, wl.items, dev, 0)
        try:
            res["batch64"] = batch64(torch, run, a.runs, only_stage=a.only == "batch64-stage")
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
