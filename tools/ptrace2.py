"""Two-layer phase timeline of the single-sequence persistent decode (t2s_persist1.hip),
step 8, layers 12 (group 4: attention WGs 128..143, FFN 144..159) and 13 (group 5:
attention 160..175, FFN 176..191).  Microseconds from the first layer-12 attention stamp.
attention: 0 before the x_l wait, 1 x_l ready, 2 q/k/v ready, 3 softmax numerators,
4 head output, 5 partials published.  FFN: 0 start, 1 woke / x_l ready, 2 head partials
summed, 6 h1 ready, 3 FFN1 done, 4 FFN2 partials published.

Under GENIE_PERSIST_GROUPS=G (fewer layer groups, as a decode lane's 3) layer l runs on
group l % G, workgroups 32 (l % G) ..; a group that also owns layer 0 keeps only the
stamps of step 9's layer 0 (the kernel probes that one last), so its layer is left out
(G = 3: layer 12).  The FFN workgroups of group 1 also compute the logits, whose
step-end trace overwrites their stamps 0..2: when layer 13 runs there (G = 3), read hop A
to the h1 row, attention s5 -> FFN s6."""
import os
import sys
sys.path.insert(0, ".")
import numpy as np
from genie_tts_amd import synth
from genie_tts_amd.engine import Engine, make_sampler

G = max(3, min(8, int(os.environ.get("GENIE_PERSIST_GROUPS", "8"))))
w = synth.synthetic_character("v2")
e = Engine({k: w[k] for k in ("t2s_encoder", "t2s")}, "v2")
e.set_option("ptrace", 1)
ref = synth.synth_phones(48, "r"); txt = synth.synth_phones(45, "t"); ssl = synth.synth_ssl(264)
e.set_timing(True)
for rep in range(3):
    e.t2s_generate([(ref, txt, None, None, ssl)], make_sampler(force_steps=81))
print("decode ms", e.timing()[2])
tr = e.ptrace().astype(np.int64)
layers = [l for l in (12, 13) if l % G != 0]
base = {l: 32 * (l % G) for l in layers}
t0 = tr[base[layers[0]]:base[layers[0]] + 16, 0].min()
rows = [(f"{role}{l}", base[l] + off) for l in layers for role, off in (("attn", 0), ("ffn", 16))]
for nm, b in rows:
    t = (tr[b:b + 16, :8] - t0) * 10 / 1000.0
    print(f"{nm:6s} " + "  ".join(f"s{i} {t[:, i].min():6.2f}/{np.median(t[:, i]):6.2f}/{t[:, i].max():6.2f}"
                                for i in range(8) if -1e5 < t[:, i].max() < 1e5))
if "--wg" in sys.argv:   # per-workgroup stamps of the FFN groups (late-publisher hunt)
    for nm, b in rows:
        if not nm.startswith("ffn"):
            continue
        t = (tr[b:b + 16, :8] - t0) * 10 / 1000.0
        for j in range(16):
            print(f"{nm} wg{j:2d} " + " ".join(f"s{i} {t[j, i]:7.2f}" for i in (0, 1, 2, 6, 3, 4)))
