"""Nucleus sampling (top_p) oracle: a torch restatement of the sampler with GPT-SoVITS's
logits_to_probs order (include/genie_engine.h, the gsv_sampler block):

  1. repetition penalty on the history tokens -> l (float32);
  2. top_p < 1: p = softmax(l) before the temperature; tokens ordered by l descending, equal
     l by ascending index (a stable descending sort); S_i the inclusive cumulative sum of p
     in that order; token i removed iff S_i > top_p and i is not first in the order;
  3. l / temperature, the top-k threshold with multiplicity, softmax, argmax(p / q).

The cut is decided from S_i in float64 on the float32 penalised logits, compared with
float32(top_p) widened to double.  A float32 sum of up to 1025 non-negative terms of total
<= 1 errs by at most 1024 * 2^-24 ~ 6.1e-5 in any order, so a float32 implementation must
agree whenever margin() >= MARGIN = 1e-4; tests assert that of their inputs.
"""
from typing import Sequence, Tuple

import numpy as np
import torch

from oracle import restate as R

MARGIN = 1e-4


def penalised(logits, hist, repetition_penalty: float = 1.35) -> torch.Tensor:
    l = torch.as_tensor(np.asarray(logits, np.float32)).clone()
    h = torch.as_tensor(np.asarray(hist, np.int64))
    g = l[h]
    l[h] = torch.where(g < 0, g * repetition_penalty, g / repetition_penalty)
    return l


def cum_probs(l: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(order, S): the stable descending order of l and the float64 inclusive cumulative
    softmax in that order."""
    order = torch.sort(l, descending=True, stable=True).indices
    p = torch.softmax(l.double(), dim=-1)
    return order, torch.cumsum(p[order], dim=0)


def survivors(l: torch.Tensor, top_p: float) -> torch.Tensor:
    """Boolean mask over the vocabulary of the tokens step 2 keeps."""
    order, S = cum_probs(l)
    rem = S > float(np.float32(top_p))
    rem[0] = False
    keep = torch.ones_like(rem)
    keep[order] = ~rem
    return keep


def margin(logits, hist, top_p: float, repetition_penalty: float = 1.35) -> float:
    """min_i |S_i - top_p| over the row's float64 cumulative sums."""
    _, S = cum_probs(penalised(logits, hist, repetition_penalty))
    return float((S - float(np.float32(top_p))).abs().min())


def pick_top_p(rows: Sequence[tuple], target: float, repetition_penalty: float = 1.35) -> float:
    """rows: (logits, hist) pairs.  Of target + k * 1e-3, |k| <= 20 (inside (0, 1)), the
    candidate with the largest worst-row margin."""
    Ss = [cum_probs(penalised(lg, h, repetition_penalty))[1] for lg, h in rows]
    best, best_m = None, -1.0
    for k in range(-20, 21):
        c = float(np.float32(target + k * 1e-3))
        if not 0.0 < c < 1.0:
            continue
        m = min(float((S - c).abs().min()) for S in Ss)
        if m > best_m:
            best, best_m = c, m
    return best


def sample(logits, hist, q, top_k: int = 15, temperature: float = 1.0, repetition_penalty: float = 1.35,
           top_p: float = 1.0) -> Tuple[int, int]:
    """(token, argmax of the raw logits); equals oracle.restate.sample at top_p == 1."""
    raw = torch.as_tensor(np.asarray(logits, np.float32))
    l = penalised(raw, hist, repetition_penalty)
    if top_p < 1.0:
        l = torch.where(survivors(l, top_p), l, torch.tensor(float("-inf")))
    l = l / temperature
    thr = torch.topk(l, top_k).values[-1]
    l = torch.where(l < thr, torch.tensor(float("-inf")), l)
    p = torch.softmax(l, dim=-1)
    return int(torch.argmax(p / torch.as_tensor(q))), int(torch.argmax(raw))


def restate_sample(logits, hist, q, top_k=15, temperature=1.0, repetition_penalty=1.35) -> Tuple[int, int]:
    cfg = R.SamplerCfg(top_k=top_k, temperature=temperature, repetition_penalty=repetition_penalty)
    return R.sample(torch.as_tensor(np.asarray(logits, np.float32)), torch.as_tensor(np.asarray(hist, np.int64)),
                    torch.as_tensor(q), cfg)


def seen_bits(hist) -> np.ndarray:
    bits = np.zeros(33, np.uint32)
    for t in hist:
        bits[int(t) >> 5] |= np.uint32(1 << (int(t) & 31))
    return bits.view(np.int32)
