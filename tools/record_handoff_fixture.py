"""Record tests/golden/handoff_halves.npz: what the single-sequence persistent decode
(k_decode_persist1) computes for the smallest prompt (R = 12, S = 10, H = 41: N0 = 42)
in 9 forced steps -- the yardstick of tests/test_handoff_halves_gpu.py.  Run it on the GPU
at the commit whose hand-off arithmetic is the reference, before the kernel changes:

    python tools/record_handoff_fixture.py [--out PATH] [--force]

Holds the greedy tokens, the top-k 5 sampled tokens (seed 1234), the K and V rows
[0, N0 + 9) of layers 0, 11 and 23 after the greedy run, and a SHA-256 of every layer's K
and V bytes (all rows the engine returns) after the greedy and after the sampled run.
Records and does nothing else; refuses to overwrite an existing file without --force."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

R_, S_, H_, STEPS, TAG = 12, 10, 41, 9, "p12"
N0 = R_ + S_ + H_ // 2
LAYERS = (0, 11, 23)


def samplers():
    from genie_tts_amd.engine import make_sampler
    return (make_sampler(force_steps=STEPS),
            make_sampler(top_k=5, greedy=False, seed=1234, force_steps=STEPS))


def kv_of(eng, seq=0):
    """([K rows, V rows] per layer as numpy, [sha256 of K, of V] per layer)."""
    rows, sha = [], []
    for layer in range(24):
        k, v = (t.cpu().numpy() for t in eng.t2s_read_kv(layer, seq))
        rows.append((k, v))
        sha.append((hashlib.sha256(k.tobytes()).hexdigest(), hashlib.sha256(v.tobytes()).hexdigest()))
    return rows, sha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "handoff_halves.npz"))
    ap.add_argument("--force", action="store_true", help="overwrite an existing fixture")
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{args.out} exists (--force overwrites it)")
    from genie_tts_amd import synth
    from genie_tts_amd.engine import Engine
    from tests.common import t2s_inputs
    w = synth.synthetic_character("v2")
    eng = Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")
    try:
        eng.set_option("persist", 1)
        inp = t2s_inputs(R=R_, S=S_, H=H_, tag=TAG)
        greedy, sampled = samplers()
        t0 = eng.counter("persist_timeouts")
        n0 = eng.counter("persist_launches")
        tok_s = eng.t2s_generate([inp], sampled)[0]
        _, sha_s = kv_of(eng)
        tok_g = eng.t2s_generate([inp], greedy)[0]
        rows, sha_g = kv_of(eng)
        assert eng.counter("persist_timeouts") == t0 and eng.counter("persist_launches") == n0 + 2
    finally:
        eng.close()
    assert all(k.shape[0] >= N0 + STEPS for k, _ in rows), [k.shape for k, _ in rows]
    out = dict(tokens_greedy=tok_g.astype(np.int64), tokens_sampled=tok_s.astype(np.int64),
               kv_rows=np.int64(rows[0][0].shape[0]), sha_greedy=np.array(sha_g), sha_sampled=np.array(sha_s))
    for layer in LAYERS:
        out[f"k{layer}"] = rows[layer][0][:N0 + STEPS]
        out[f"v{layer}"] = rows[layer][1][:N0 + STEPS]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, greedy {tok_g.tolist()}, sampled {tok_s.tolist()}, "
          f"{int(out['kv_rows'])} K/V rows")


if __name__ == "__main__":
    main()
