"""GPU: every instantiation of the attention kernel (csrc/attention.hip: ring depth 2 | 3 | 4, 4 | 8 waves, DMA issue spread or not)
against float64 softmax attention, at the key counts where the K loop changes regime, ragged query blocks, the engine's strided
layouts, and with everything the kernel must not read poisoned and everything it must not write watched.

Two gates on every comparison, both against float64 (oracle/attention_ref.py):
  (a) every element within attention_bound = 2^-11 * (2 |want| + softmax(s) @ |V|) + 1e-7, the contract's worst case;
  (b) whole-tensor relative L2 <= 1.5 x that of attention_emulated, the kernel's recurrence in plain fp32 on the same inputs
      (kernel and emulation differ only in MFMA accumulation order and the hardware exp2, far below fp16 rounding).
tests/test_attention_cpu.py shows that a correct implementation keeps to 0.75 of (a) on these same inputs."""
import ctypes as C
import pytest
import torch
from oracle import attention_ref as A

pytestmark = pytest.mark.gpu

SCALE = 0.125
VARIANTS = [(2, 0, 1), (3, 0, 1), (4, 0, 1), (2, 1, 1), (3, 1, 1), (4, 1, 1), (3, 0, 0), (3, 1, 0)]      # (NS, NW8, SPREAD)
SENTINEL = 0x7E01           # an fp16 NaN: a cell the kernel should have written and did not shows as non-finite, too
NAN_ROWS = 64               # poisoned K / V rows behind the last batch's last key: one whole tile of them
WORST = {}                  # variant -> [worst element / bound, worst rel L2 / emulation's]: printed for the record
_REFS = {}                  # inputs and float64 reference per case, shared by the variants


def _lib():
    from contexture_nerf_amd import _lib as L
    return L, L.load()


def _case(B, Sq, Skv, heads, lazy=8.0):
    key = (B, Sq, Skv, heads, lazy)
    if key not in _REFS:
        q, k, v = A.random_qkv(B, Sq, Skv, heads, A.case_seed(B, Sq, Skv, heads))
        _REFS[key] = (q, k, v, A.reference(q, k, v, SCALE, lazy))
    return _REFS[key]


def _poison(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float16)


def _sentinel(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int16).view(torch.float16)


def _launch(dev, q, k, v, layout="plain", scale=SCALE):
    """One call of ctx_attention_f16 on q, k, v [B, S, heads*64] (CPU fp16) stored as `layout`:
      plain    three tensors, strides C                           packed   one [B*S, 3C] buffer, strides 3C (self-attention)
      kv2c     q stride C, K|V one [Skv, 2C] buffer (B = 1)       wide     K|V at column 6C of a [B*L, 10C] buffer, stride 10C
      ostride  plain inputs, O rows C + 64 apart
    Every K / V buffer carries NAN_ROWS rows of NaN behind the last valid row and NaN in every column that belongs to nobody; O is
    pre-filled with a NaN sentinel and has 8 more rows (and, for ostride, 64 more columns) than the kernel may write.  Returns
    O [B, Sq, C] on the CPU after asserting that every sentinel cell is bit-unchanged; the views the references should read are
    returned too (they alias the host images of the device buffers, so the references see the strides the kernel saw)."""
    L, lib = _lib()
    B, Sq, Cc = q.shape
    Skv = k.shape[1]
    heads = Cc // 64
    ocols = Cc + 64 if layout == "ostride" else Cc
    if layout == "packed":
        assert Sq == Skv
        buf = _poison(B * Sq + NAN_ROWS, 3 * Cc)
        buf[:B * Sq] = torch.cat([q, k, v], -1).view(B * Sq, 3 * Cc)
        bufs = [buf]
        views = [(0, 0, 3 * Cc), (0, Cc, 3 * Cc), (0, 2 * Cc, 3 * Cc)]          # (buffer, column offset, row stride)
    elif layout == "kv2c":
        assert B == 1
        buf = _poison(Skv + NAN_ROWS, 2 * Cc)
        buf[:Skv] = torch.cat([k, v], -1)[0]
        bufs = [q.reshape(B * Sq, Cc).clone(), buf]
        views = [(0, 0, Cc), (1, 0, 2 * Cc), (1, Cc, 2 * Cc)]
    elif layout == "wide":
        buf = _poison(B * Skv + NAN_ROWS, 10 * Cc)
        buf[:B * Skv, 6 * Cc:8 * Cc] = torch.cat([k, v], -1).view(B * Skv, 2 * Cc)
        bufs = [q.reshape(B * Sq, Cc).clone(), buf]
        views = [(0, 0, Cc), (1, 6 * Cc, 10 * Cc), (1, 7 * Cc, 10 * Cc)]
    else:
        kb, vb = _poison(B * Skv + NAN_ROWS, Cc), _poison(B * Skv + NAN_ROWS, Cc)
        kb[:B * Skv] = k.reshape(B * Skv, Cc); vb[:B * Skv] = v.reshape(B * Skv, Cc)
        bufs = [q.reshape(B * Sq, Cc).clone(), kb, vb]
        views = [(0, 0, Cc), (1, 0, Cc), (2, 0, Cc)]
    dbufs = [b.to(dev) for b in bufs]
    o = _sentinel(B * Sq + 8, ocols).to(dev)
    ptr = [C.c_void_p(dbufs[i].data_ptr() + 2 * off) for i, off, _ in views]
    rc = lib.ctx_attention_f16(ptr[0], ptr[1], ptr[2], B, Sq, Skv, heads, views[0][2], views[1][2], scale, L.ptr(o), ocols, None, L.stream())
    torch.cuda.synchronize()
    L.check(rc)
    oc = o.cpu()
    bits = oc.view(torch.int16)
    assert bool((bits[B * Sq:] == SENTINEL).all()), "rows behind B*Sq of O were written"
    assert bool((bits[:, Cc:] == SENTINEL).all()), "columns behind heads*64 of O were written"
    hv = [bufs[i][:B * S, off:off + Cc].view(B, S, Cc) for S, (i, off, st) in zip((Sq, Skv, Skv), views)]
    assert all(h.stride(1) == st and h.stride(0) == h.shape[1] * st for h, (_, _, st) in zip(hv, views))
    return oc[:B * Sq, :Cc].reshape(B, Sq, Cc), hv


def _gate(o, q, k, v, what, lazy=8.0, ref=None, variant=None, scale=SCALE):
    f = A.compare(o, q, k, v, scale, lazy, ref)
    ratio = f["rel"] / f["rel_emu"] if f["rel_emu"] > 0 else (0.0 if f["rel"] == 0 else float("inf"))
    print(f"{what}: element/bound {f['elem']:.3f}, rel L2 {f['rel']:.3e} vs emulation {f['rel_emu']:.3e} (x{ratio:.2f})")
    if variant is not None:
        w = WORST.setdefault(variant, [0.0, 0.0])
        w[0] = max(w[0], f["elem"]); w[1] = max(w[1], ratio)
    assert f["finite"], f"{what}: non-finite output"
    assert f["elem"] <= 1.0, f"{what}: an element is at {f['elem']:.3f} of the bound"
    assert f["rel"] <= 1.5 * f["rel_emu"], f"{what}: rel L2 {f['rel']:.3e} > 1.5 x the emulation's {f['rel_emu']:.3e}"
    return f


def _tune(variant, lazy=-1.0):
    _lib()[1].ctx_attention_tune(variant[0], variant[1], variant[2], lazy)


def _clear():
    _lib()[1].ctx_attention_tune(-1, -1, -1, -1.0)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda t: "ns%d_nw%d_spread%d" % (t[0], 8 if t[1] else 4, t[2]))
def test_every_variant_at_pipeline_boundaries(dev, variant):
    """Key counts 1 .. 320: one ragged tile alone, exactly one tile (the drain loop is the only loop), ntiles == NS-1 and == NS
    (the steady loop runs zero times or once), a one-key ragged tile behind 1 - 4 full ones; query counts that leave a ragged wave
    and waves that own no query at all; a planted dominant key per position class."""
    try:
        _tune(variant)
        for B, Sq, Skv, heads in A.grid_cases(variant[1]):
            q, k, v, ref = _case(B, Sq, Skv, heads)
            o, _ = _launch(dev, q, k, v)
            _gate(o, q, k, v, f"{variant} B{B} Sq{Sq} Skv{Skv} heads{heads}", ref=ref, variant=variant)
    finally:
        _clear()
    print("worst so far (element/bound, rel L2 / emulation):", {k: [round(x, 3) for x in w] for k, w in WORST.items()})


@pytest.mark.parametrize("variant", [(3, 0, 1), (3, 1, 1), (4, 0, 1), (2, 1, 1)], ids=lambda t: "ns%d_nw%d" % (t[0], 8 if t[1] else 4))
@pytest.mark.parametrize("layout", ["packed", "kv2c", "wide7", "wide77", "ostride"])
def test_engine_layouts(dev, variant, layout):
    """The strides the engine passes (unet.hip: run_transformer), which the plain tests never do: Q|K|V packed in one [M, 3C] buffer;
    reference-only attention's [S+Sr, 2C] K|V with q_stride C, one batch per call; cross-attention's K|V at a column offset of the
    wide kv_all buffer; and an output whose rows are further apart than heads*64."""
    if layout == "packed":
        shape = (2, 129, 129, 3)
    elif layout == "kv2c":
        shape = (1, 100, 193, 3)         # S = 100 image tokens + Sr = 93 reference tokens
    elif layout.startswith("wide"):
        shape = (2, 129, int(layout[4:]), 3)
    else:
        shape = (2, 129, 193, 3)
    q, k, v = A.random_qkv(*shape, A.case_seed(*shape))
    try:
        _tune(variant)
        o, (qv, kv, vv) = _launch(dev, q, k, v, layout[:4] if layout.startswith("wide") else layout)
    finally:
        _clear()
    _gate(o, qv, kv, vv, f"{variant} {layout}", variant=variant)


def test_default_dispatch_with_a_ragged_eight_wave_block(dev):
    """No override: Sq = Skv = 1030 takes the 8-wave kernel by the size rule, and its fifth workgroup owns 6 queries: seven of its
    eight waves own none, yet move their DMA pieces and meet every barrier."""
    _clear()
    shape = (1, 1030, 1030, 2)
    q, k, v, ref = _case(*shape)
    o, _ = _launch(dev, q, k, v)
    _gate(o, q, k, v, "default dispatch 1030 x 1030", ref=ref)


def test_near_one_hot_rows(dev):
    """|score * scale| up to ~70: log2 scores far apart, so most of P underflows in fp16 and the rescale factor reaches 0."""
    shape = (1, 129, 193, 3)
    q, k, v = A.sharp_qkv(*shape, seed=11)
    ref = A.reference(q, k, v, SCALE)
    try:
        for variant in VARIANTS:
            _tune(variant)
            o, _ = _launch(dev, q, k, v)
            _gate(o, q, k, v, f"{variant} near-one-hot", ref=ref, variant=variant)
    finally:
        _clear()


@pytest.mark.parametrize("lazy", [0.0, 8.0, 12.0])
def test_creeping_maximum_at_each_threshold(dev, lazy):
    """The input of test_unet_gpu.py::test_attention_creeping_maximum_lazy_rescale with the threshold set by the override: never
    stale (0), the default (8), and the largest the library accepts (12: P up to 4096)."""
    q, k, v = A.creeping_qkv()
    ref = A.reference(q, k, v, SCALE, lazy)
    outs = []
    try:
        for variant in VARIANTS:
            _tune(variant, lazy)
            o, _ = _launch(dev, q, k, v)
            _gate(o, q, k, v, f"{variant} creeping maximum, lazy {lazy}", lazy=lazy, ref=ref, variant=variant)
            outs.append(o)
    finally:
        _clear()
    if lazy > 0:        # the threshold is in force: the stale maximum rounds P differently from the textbook recurrence
        try:
            _tune(VARIANTS[1], 0.0)
            o0, _ = _launch(dev, q, k, v)
        finally:
            _clear()
        assert not torch.equal(o0, outs[1])
        assert float(((o0.double() - outs[1].double()).abs() / ref[1]).max()) <= 1.0


IDENTITY_SHAPES = [(2, 1031, 1031, 5), (1, 257, 320, 3), (2, 40, 193, 1)]


def test_variants_are_bit_identical_and_repeatable(dev):
    """Every wave runs the same 32 queries through the same tile sequence whatever the ring depth, the workgroup width or the DMA issue
    order, and the lazy decision is per wave: for fixed inputs all eight variants return the same bits.  On the shape with several
    workgroups per CU each variant is launched three times and must repeat itself bit for bit (the race screen: an early LDS read or
    refill shows in some launches only)."""
    try:
        for shape in IDENTITY_SHAPES:
            q, k, v, ref = _case(*shape)
            outs = {}
            for variant in VARIANTS:
                _tune(variant)
                o, _ = _launch(dev, q, k, v)
                if shape == IDENTITY_SHAPES[0]:
                    for rep in (1, 2):
                        again, _ = _launch(dev, q, k, v)
                        assert torch.equal(again.view(torch.int16), o.view(torch.int16)), \
                            f"{variant} {shape}: launch {rep} differs from launch 0 in {int((again.view(torch.int16) != o.view(torch.int16)).sum())} elements"
                outs[variant] = o
            _gate(outs[VARIANTS[1]], q, k, v, f"{VARIANTS[1]} {shape}", ref=ref, variant=VARIANTS[1])
            for variant in VARIANTS:
                n = int((outs[variant].view(torch.int16) != outs[VARIANTS[1]].view(torch.int16)).sum())
                print(f"{shape} {variant} vs {VARIANTS[1]}: {n} elements differ")
                assert n == 0, f"{shape}: {variant} differs from {VARIANTS[1]} in {n} elements"
    finally:
        _clear()


def test_bad_arguments_are_refused_without_a_launch(dev):
    L, lib = _lib()
    B, Sq, Skv, heads = 2, 33, 65, 3
    Cc = heads * 64
    q = torch.randn(2 * B * Sq, Cc, device=dev).half(); k = torch.randn(2 * B * Skv, Cc, device=dev).half(); v = torch.randn(2 * B * Skv, Cc, device=dev).half()
    o = _sentinel(2 * B * Sq, Cc).to(dev)
    good = dict(Q=L.ptr(q), K=L.ptr(k), V=L.ptr(v), B=B, Sq=Sq, Skv=Skv, heads=heads, qs=Cc, kvs=Cc, O=L.ptr(o), os=Cc)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ctx_attention_f16(a["Q"], a["K"], a["V"], a["B"], a["Sq"], a["Skv"], a["heads"], a["qs"], a["kvs"], SCALE, a["O"], a["os"], None, L.stream())

    bad = [dict(Q=None), dict(K=None), dict(V=None), dict(O=None),
           dict(qs=Cc + 4), dict(kvs=Cc + 4), dict(os=Cc + 2),                      # strides: multiples of 8 / 8 / 4 elements
           dict(qs=Cc - 8), dict(kvs=Cc - 8), dict(os=Cc - 4),                      # and no smaller than heads*64
           dict(B=0), dict(Sq=0), dict(Skv=0), dict(heads=0), dict(B=-1), dict(Sq=-1), dict(Skv=-1), dict(heads=-1)]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0, f"{kw} was accepted"
        with pytest.raises(L.CtxError, match="attention"):
            L.check(rc)
    torch.cuda.synchronize()
    assert bool((o.cpu().view(torch.int16) == SENTINEL).all()), "a refused call wrote to O"
    L.check(call())                                                                  # and the same arguments, all good, run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o[:B * Sq].float()).all()) and bool((o[B * Sq:].cpu().view(torch.int16) == SENTINEL).all())
