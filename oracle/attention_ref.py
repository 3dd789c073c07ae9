"""The contract of csrc/attention.hip, restated in plain torch on the CPU (test infrastructure only).

O = softmax(Q K^T * scale) V over [B, S, heads*64] views of fp16 buffers (any row / batch strides, head_dim 64).

  attention_f64       the operation itself in float64: what every comparison is made against.
  attention_emulated  the kernel's own recurrence in fp32: 64-key tiles; per 32-query wave one decision whether the subtracted
                      maximum follows the running one (only when some row of the wave has moved by more than `lazy` log2 units);
                      P = exp2(s*c - m) rounded to fp16; the row sums taken over that rounded P; O and l rescaled only when the
                      maximum moved; fp16 output.  It differs from the kernel only in the accumulation order inside a product
                      and in the hardware exp2, both far below the fp16 rounding of P.
  attention_bound     the worst-case error per output element that this contract allows:
                          2^-11 * (2 |want| + softmax(s) @ |V|) + 1e-7
                      one half-ulp (2^-11 relative) for the fp16 output; one for the normaliser, a sum of P each rounded to fp16
                      (relative error of a sum of positive terms <= the largest relative error of a term); one half-ulp per
                      term of P in the product, which weights |V| with the softmax.  Rounding of the scores (fp16 products are
                      exact in fp32, 64 additions of 2^-24), of exp2 (<= 2 ulp of fp32) and of the fp32 accumulation are >= 2^10
                      times smaller and sit inside the slack between 2^-11 and what an implementation actually reaches
                      (tests/test_attention_cpu.py holds the emulation to 0.75 of the bound).

The input families of tests/test_attention_{cpu,gpu}.py live here too, so both files see the same tensors."""
import math
import torch

LOG2E = 1.4426950408889634
TILE = 64          # keys per tile
WAVE = 32          # queries that share one rescale decision


def _heads(x):
    """[B, S, heads*64] view (any strides) -> [B, heads, S, 64]."""
    B, S, C = x.shape
    assert C % 64 == 0
    return x.reshape(B, S, C // 64, 64).transpose(1, 2)


def _merge(o):
    """[B, heads, S, 64] -> [B, S, heads*64]."""
    B, H, S, _ = o.shape
    return o.transpose(1, 2).reshape(B, S, H * 64)


def attention_f64(q, k, v, scale):
    qh, kh, vh = (_heads(t).double() for t in (q, k, v))
    return _merge(torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh)


def attention_bound(q, k, v, scale):
    qh, kh, vh = (_heads(t).double() for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    return 2.0 ** -11 * (2.0 * _merge(p @ vh).abs() + _merge(p @ vh.abs())) + 1e-7


def attention_emulated(q, k, v, scale, lazy=8.0):
    qh, kh, vh = (_heads(t).float() for t in (q, k, v))
    B, H, Sq, _ = qh.shape
    Skv = kh.shape[2]
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)      # the kernel's fp32 scale * log2(e)
    nw = (Sq + WAVE - 1) // WAVE
    qp = torch.zeros(B, H, nw * WAVE, 64)
    qp[:, :, :Sq] = qh                               # the rows a ragged wave does not own carry zeros, as in the kernel
    qp = qp.view(B, H, nw, WAVE, 64)
    m = torch.full((B, H, nw, WAVE), -math.inf)
    o = torch.zeros(B, H, nw, WAVE, 64)
    l = torch.zeros(B, H, nw, WAVE)
    for k0 in range(0, Skv, TILE):
        kt = kh[:, :, None, k0:k0 + TILE]            # [B, H, 1, <=64, 64]
        vt = vh[:, :, None, k0:k0 + TILE]
        s = qp @ kt.transpose(-1, -2)                # fp32 scores, unscaled
        cand = torch.maximum(m, s.max(-1).values * c)
        move = (cand > m + lazy).any(-1, keepdim=True)                      # one decision per wave
        m_new = torch.where(move, cand, m)
        t = (s.double() * c.double() - m_new[..., None].double()).float()   # one rounding: the kernel's fused multiply-add
        p = torch.exp2(t).half().float()
        alpha = torch.where(move, torch.exp2(m - m_new), torch.ones_like(m))
        o = o * alpha[..., None] + p @ vt
        l = l * alpha + p.sum(-1)
        m = m_new
    out = (o * (1.0 / l)[..., None]).half()
    return _merge(out.view(B, H, nw * WAVE, 64)[:, :, :Sq])


def compare(got, q, k, v, scale, lazy=8.0, ref=None):
    """Figures of the two gates for a kernel output `got` (fp16, [B, Sq, heads*64]), both against float64:
    elem = max |got - want| / attention_bound (gate: <= 1), rel = relative L2 of got, rel_emu = relative L2 of the emulation
    (gate: rel <= 1.5 rel_emu).  `ref` caches (want, bound, rel_emu) for inputs that several tests share."""
    if ref is None:
        ref = reference(q, k, v, scale, lazy)
    want, bound, rel_emu = ref
    err = (got.double().cpu() - want).abs()
    return dict(elem=float((err / bound).max()), rel=float(err.norm() / want.norm()), rel_emu=rel_emu,
                finite=bool(torch.isfinite(got.float()).all()))


def reference(q, k, v, scale, lazy=8.0):
    want = attention_f64(q, k, v, scale)
    emu = attention_emulated(q, k, v, scale, lazy).double()
    return want, attention_bound(q, k, v, scale), float((emu - want).norm() / want.norm())


# ------------------------------------------------------------------------------------------------ input families

def planted_positions(Skv):
    """One key per position class: key 0, last key of tile 0, first key of tile 1, first key of the ragged tile, key Skv-1."""
    pos = [0, TILE - 1, TILE, Skv - 1]
    if Skv % TILE:
        pos.append(Skv // TILE * TILE)
    return sorted({p for p in pos if p < Skv})


def plant(q, k, gain=3.0):
    """k[j] = gain * q[i] per head for the position classes of j: key j then dominates query i (score gain*|q|^2*scale ~ 24 against
    N(0, 1) for the others), so a dropped, duplicated or misplaced key moves that output row by O(1).  Returns the (i, j) pairs."""
    B, Sq, _ = q.shape
    pairs = []
    for n, j in enumerate(planted_positions(k.shape[1])):
        i = (7 * n + 3) % Sq
        k[:, j] = (gain * q[:, i].float()).half()
        pairs.append((i, j))
    return pairs


V_FLOOR = 0.25


def floor_v(v):
    """|v| >= V_FLOOR, signs kept.  Where one key dominates a row, every other P lies below 2^-14 of the subtracted maximum: fp16
    rounds those absolutely (to 2^-25 of the maximum, or to zero), not to 2^-11 of themselves, which is worth up to
    Skv * 2^-25 * max|V| ~ 1e-5 per output.  attention_bound models relative rounding only, and its absolute term covers that only
    while the bound is not itself that small, i.e. while the dominant key's V is not ~0 in the column (|v| < 3e-4: about one
    element in 4000 of a normal V).  With |V| >= 0.25 the bound is >= 2^-11 * 0.25 = 1.2e-4 everywhere and the contract's relative
    model holds; the families without dominant keys keep a plain normal V."""
    return torch.where(v.abs() < V_FLOOR, torch.copysign(torch.full_like(v, V_FLOOR), v), v)


def random_qkv(B, Sq, Skv, heads, seed, planted=True):
    g = torch.Generator().manual_seed(seed)
    C = heads * 64
    q = torch.randn(B, Sq, C, generator=g).half()
    k = torch.randn(B, Skv, C, generator=g).half()
    v = torch.randn(B, Skv, C, generator=g).half()
    if planted:
        plant(q, k)
        v = floor_v(v)
    return q, k, v


SHARP_GAIN = 2.74       # |score * scale| reaches ~60 (|q|^2 ~ 64 per head, times gain^2 / 8)


def sharp_qkv(B, Sq, Skv, heads, seed, gain=SHARP_GAIN):
    """Near-one-hot rows: q and k both scaled by `gain`, so score*scale ~ N(0, gain^4) (a spread of +-25) and the planted keys
    k[j] = q[i] reach gain^2 * 64 / 8 ~ 60; the log2 scores span far more than fp16's exponent range below the maximum."""
    q, k, v = random_qkv(B, Sq, Skv, heads, seed, planted=False)
    q = (q.float() * gain).half()
    k = (k.float() * gain).half()
    plant(q, k, gain=1.0)
    return q, k, floor_v(v)


def creeping_qkv():
    """Scores of one query rise a little with every key, so the subtracted maximum stays stale for several tiles and P runs up to
    2^lazy before a rescale; a row of the other head jumps once; rows that never move and a ragged last tile in the same workgroup."""
    B, S, Skv, heads = 1, 192, 1000, 2
    g = torch.Generator().manual_seed(4)
    q = torch.randn(B, S, heads * 64, generator=g).half()
    k = (0.05 * torch.randn(B, Skv, heads * 64, generator=g)).half()
    v = torch.randn(B, Skv, heads * 64, generator=g).half()
    ramp = torch.linspace(0.0, 6.0, Skv)                                    # log2-scores creep up by ~0.4 per 64-key tile ...
    k[0, :, :64] += (ramp[:, None] * q[0, 3:4, :64].float() / q[0, 3, :64].float().pow(2).sum() * 8 / 1.4427).half()
    k[0, 700, 64:] = q[0, 9, 64:] * 5                                       # ... and one row of the other head jumps once
    return q, k, v


SKV = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 320)


def grid_cases(nw8):
    """(B, Sq, Skv, heads) met by every kernel variant: every key count twice, against query counts 1 / 33 / 129 (one lane, a
    ragged second wave, a ragged second workgroup) and, for the 8-wave kernels, 257 (a second workgroup that owns one query) and 40
    (six of eight waves own no query); heads and batch alternate."""
    cases = []
    for i, Skv in enumerate(SKV):
        heads, B = (1, 3)[i % 2], (1, 2)[(i // 2) % 2]
        cases.append((B, (1, 33, 129)[i % 3], Skv, heads))
        cases.append((3 - B, (257, 40)[i % 2] if nw8 else (33, 129, 1)[i % 3], Skv, 4 - heads))
    return cases


def case_seed(B, Sq, Skv, heads):
    return ((B * 1000 + Sq) * 1000 + Skv) * 10 + heads
