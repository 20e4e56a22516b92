"""Record tests/golden/decode_abandon.json: what the engine leaves after the calls of
tests/test_decode_abandon_gpu.py::test_abandoned_launch_leaves_no_trace (abandon_calls there:
persist1_f16_limit doubled from 1 until a persistent launch no longer trips, then one clean
generate) -- for every call the tokens, whether the launch tripped, and the SHA-256 of the K and V
rows of layers 0, 11 and 23.  Run it on the GPU at the commit whose behaviour is the reference,
before the kernel changes:

    python tools/record_decode_abandon_fixture.py [--out PATH] [--force]

Records and does nothing else; refuses to overwrite an existing file without --force."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decode_abandon.json"))
    ap.add_argument("--force", action="store_true", help="overwrite an existing fixture")
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{args.out} exists (--force overwrites it)")
    from genie_tts_amd import synth
    from genie_tts_amd.engine import Engine
    from tests.test_decode_abandon_gpu import abandon_calls
    w = synth.synthetic_character("v2")
    eng = Engine({"t2s_encoder": w["t2s_encoder"], "t2s": w["t2s"]}, "v2")
    try:
        eng.set_option("persist", 1)
        out = {"whole_chip": abandon_calls(eng, False), "two_lanes": abandon_calls(eng, True)}
    finally:
        eng.close()
    for name, rec in out.items():
        print(name, [(c["limit"], c["tripped"]) for c in rec["calls"]], "timeouts", rec["timeouts"],
              "tokens", rec["graphs"])
        assert rec["timeouts"] == 0 and not rec["calls"][-1]["tripped"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
