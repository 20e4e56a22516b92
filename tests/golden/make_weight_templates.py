#!/usr/bin/env python3
"""Generate tests/golden/weight_templates.json: the initializer tables (names and
shapes only, no values) of the reference's template graphs, read with
genie_tts_amd.onnx_table.  tests/test_weights_spec.py compares the weight specs to them.
Usage: python tests/golden/make_weight_templates.py DATA_DIR
       (DATA_DIR: src/genie_tts/Data of a reference checkout)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from genie_tts_amd.onnx_table import read_initializer_table  # noqa: E402

GRAPHS = [
    "v2/Models/t2s_first_stage_decoder_fp32.onnx",
    "v2/Models/t2s_stage_decoder_fp32.onnx",
    "v2/Models/t2s_encoder_fp32.onnx",
    "v2/Models/vits_fp32.onnx",
    "v2ProPlus/Models/vits_fp32.onnx",
    "v2ProPlus/Models/prompt_encoder_fp32.onnx",
]


def main():
    data = sys.argv[1]
    out = {rel: {name: [int(d) for d in entry[0]]
                 for name, entry in read_initializer_table(os.path.join(data, rel)).items()}
           for rel in GRAPHS}
    with open(os.path.join(HERE, "weight_templates.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print({rel: len(t) for rel, t in out.items()})


if __name__ == "__main__":
    main()
