"""The K/V-split form of csrc/attention.hip (12 waves: 6 query blocks x 2 key ranges), restated in plain torch on the CPU, and the
inputs tests/test_attention_split_{cpu,gpu}.py share (test infrastructure only).

The split form runs oracle/attention_ref.py's recurrence (64-key tiles, stale maximum per 32-query wave, fp16 P, row sums of the
rounded P) over two key ranges, tiles [0, ceil(ntiles/2)) and the rest, each from m = -inf, l = 0, o = 0 and each with lazy decisions
of its own, and then folds the second into the first in fp32:
    m = max(m0, m1),  o = o0 * 2^(m0 - m) + o1 * 2^(m1 - m),  l likewise,  out = fp16(o / l)
A range without tiles keeps m = -inf, l = 0, o = 0 and weighs exactly nothing."""
import math
import torch
from oracle import attention_ref as A

SKV = (1, 64, 65, 128, 129, 320, 321, 448, 576)     # half 1 empty (1, 64) | the ragged tile alone (65) | 1 + 1, 2 + 1 tiles | 3 + 2, 3 + 3 |
#                                                     4 + 3 (at a ring of 3 the steady loop runs in half 0 only) | 5 + 4
SQ = (1, 33, 191, 192, 193, 385)                    # one lane | a ragged second wave | 192 queries per workgroup - 1, exactly, + 1 |
#                                                     a third workgroup that owns one query


def split_point(Skv):
    """First key of the second range."""
    ntiles = (Skv + A.TILE - 1) // A.TILE
    return min((ntiles + 1) // 2 * A.TILE, Skv)


def _range(qp, kh, vh, c, lazy, lo, hi):
    """oracle/attention_ref.py: attention_emulated's loop over keys [lo, hi), returning the unnormalised state."""
    B, H, nw = qp.shape[:3]
    m = torch.full((B, H, nw, A.WAVE), -math.inf)
    o = torch.zeros(B, H, nw, A.WAVE, 64)
    l = torch.zeros(B, H, nw, A.WAVE)
    for k0 in range(lo, hi, A.TILE):
        kt = kh[:, :, None, k0:min(k0 + A.TILE, hi)]
        vt = vh[:, :, None, k0:min(k0 + A.TILE, hi)]
        s = qp @ kt.transpose(-1, -2)
        cand = torch.maximum(m, s.max(-1).values * c)
        move = (cand > m + lazy).any(-1, keepdim=True)
        m_new = torch.where(move, cand, m)
        t = (s.double() * c.double() - m_new[..., None].double()).float()
        p = torch.exp2(t).half().float()
        alpha = torch.where(move, torch.exp2(m - m_new), torch.ones_like(m))
        o = o * alpha[..., None] + p @ vt
        l = l * alpha + p.sum(-1)
        m = m_new
    return o, l, m


def split_emulated(q, k, v, scale, lazy=8.0):
    qh, kh, vh = (A._heads(t).float() for t in (q, k, v))
    B, H, Sq, _ = qh.shape
    Skv = kh.shape[2]
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(A.LOG2E, dtype=torch.float32)
    nw = (Sq + A.WAVE - 1) // A.WAVE
    qp = torch.zeros(B, H, nw * A.WAVE, 64)
    qp[:, :, :Sq] = qh
    qp = qp.view(B, H, nw, A.WAVE, 64)
    cut = split_point(Skv)
    o0, l0, m0 = _range(qp, kh, vh, c, lazy, 0, cut)
    o1, l1, m1 = _range(qp, kh, vh, c, lazy, cut, Skv)
    m = torch.maximum(m0, m1)
    a0 = torch.exp2(m0 - m)
    a1 = torch.where(m1 == -math.inf, torch.zeros_like(m), torch.exp2(m1 - m))
    o = o0 * a0[..., None] + o1 * a1[..., None]
    l = l0 * a0 + l1 * a1
    out = (o * (1.0 / l)[..., None]).half()
    return A._merge(out.view(B, H, nw * A.WAVE, 64)[:, :, :Sq])


def reference(q, k, v, scale, lazy=8.0):
    """oracle/attention_ref.py: reference with the split recurrence as the emulation: (want, bound, rel L2 of the emulation)."""
    want = A.attention_f64(q, k, v, scale)
    emu = split_emulated(q, k, v, scale, lazy).double()
    return want, A.attention_bound(q, k, v, scale), float((emu - want).norm() / want.norm())


def grid_cases():
    """(B, Sq, Skv, heads): every key count twice, every query count three times, batch and heads alternating."""
    cases = []
    for i, Skv in enumerate(SKV):
        B, heads = (1, 2)[i % 2], (1, 2)[(i // 2) % 2]
        cases.append((B, SQ[i % 6], Skv, heads))
        cases.append((3 - B, SQ[(i + 3) % 6], Skv, 3 - heads))
    return cases


DOMINANT_GAIN = 24.0


def dominant_qkv(B=2, Sq=193, Skv=320, heads=2, seed=17):
    """Query 5 meets k = 24 q at key 70 (range 0: keys 0 .. 191) and query 40 at key 300 (range 1): their scores stand ~200 log2
    units above everything else, so every other key of the row underflows to P = 0 in its tile and the whole other range to a weight
    2^(m_other - m) = 0 in the merge: the output row is that key's V row bit for bit.  Returns q, k, v and the (query, key) pairs."""
    q, k, v = A.random_qkv(B, Sq, Skv, heads, seed, planted=False)
    pairs = [(5, 70), (40, 300)]
    assert pairs[0][1] < split_point(Skv) <= pairs[1][1]
    for i, j in pairs:
        k[:, j] = (DOMINANT_GAIN * q[:, i].float()).half()
    return q, k, A.floor_v(v), pairs
