"""GPU: the K/V-split form of the attention kernel (csrc/attention.hip: 12 waves = 6 query blocks x 2 key ranges, rings of 2 | 3 | 4
stages per range, the partial results merged in LDS), forced with ctx_attention_tune(ns, 2, spread, lazy), through the launch harness
of tests/test_attention_gpu.py: K / V rows behind the last key and every column that belongs to nobody are NaN, O carries a sentinel
wherever the kernel must not write.

The two gates of test_attention_gpu.py against float64: (a) every element within attention_bound, unchanged; (b) whole-tensor
relative L2 <= 1.5 x that of the fp32 emulation, here of the recurrence this form runs (tests/attention_split_rule.py: two key ranges,
then the merge).  tests/test_attention_split_cpu.py shows that emulation at 0.75 of (a) on these same inputs."""
import pytest
import torch
from oracle import attention_ref as A
import attention_split_rule as R
import test_attention_gpu as G

pytestmark = pytest.mark.gpu

SCALE = G.SCALE
_REFS = {}                  # inputs and float64 reference per case, shared by the ring depths


def _case(B, Sq, Skv, heads):
    key = (B, Sq, Skv, heads)
    if key not in _REFS:
        q, k, v = A.random_qkv(B, Sq, Skv, heads, A.case_seed(B, Sq, Skv, heads))
        _REFS[key] = (q, k, v, R.reference(q, k, v, SCALE))
    return _REFS[key]


def _split(ns, spread=1, lazy=-1.0):
    G._lib()[1].ctx_attention_tune(ns, 2, spread, lazy)


def _twice(dev, q, k, v, what, layout="plain"):
    """Two launches: the same bits (the race screen: the merge reads what another wave parked, and the rings are refilled under
    the other range's feet if a barrier is missing), sentinels intact in both (checked by the harness)."""
    o, views = G._launch(dev, q, k, v, layout)
    again, _ = G._launch(dev, q, k, v, layout)
    n = int((again.view(torch.int16) != o.view(torch.int16)).sum())
    assert n == 0, f"{what}: two launches differ in {n} elements"
    return o, views


@pytest.mark.parametrize("ns", [2, 3, 4])
def test_split_form_at_range_and_pipeline_boundaries(dev, ns):
    """Key counts that leave the second range empty, with the ragged tile alone, one tile short of the first, and with a steady loop
    only in the first; query counts around the 192 of a workgroup; every ring depth."""
    try:
        _split(ns)
        for B, Sq, Skv, heads in R.grid_cases():
            q, k, v, ref = _case(B, Sq, Skv, heads)
            what = f"split ns{ns} B{B} Sq{Sq} Skv{Skv} heads{heads}"
            o, _ = _twice(dev, q, k, v, what)
            G._gate(o, q, k, v, what, ref=ref)
    finally:
        G._clear()


def test_split_form_without_issue_spread(dev):
    """spread = 0 (all DMA pieces of a tile right behind the barrier) exists at a ring of 3: same bits as the spread form."""
    shape = (2, 193, 448, 2)
    q, k, v, ref = _case(*shape)
    try:
        _split(3, 1)
        o1, _ = G._launch(dev, q, k, v)
        _split(3, 0)
        o0, _ = _twice(dev, q, k, v, "split ns3 spread0")
    finally:
        G._clear()
    G._gate(o0, q, k, v, "split ns3 spread0", ref=ref)
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))


@pytest.mark.parametrize("layout,shape", [("packed", (2, 193, 193, 2)), ("wide", (2, 193, 321, 2))])
def test_split_form_on_strided_layouts(dev, layout, shape):
    q, k, v = A.random_qkv(*shape, A.case_seed(*shape))
    try:
        _split(3)
        o, (qv, kv, vv) = _twice(dev, q, k, v, f"split {layout}", layout)
    finally:
        G._clear()
    G._gate(o, qv, kv, vv, f"split {layout}", ref=R.reference(qv, kv, vv, SCALE))


def test_dominant_key_in_one_range_only(dev):
    """A key ~200 log2 units above the rest, once in each range: the other range's weight 2^(m_other - m) underflows to 0, so the
    row is that key's V row bit for bit, whichever range holds it."""
    q, k, v, pairs = R.dominant_qkv()
    ref = R.reference(q, k, v, SCALE)
    try:
        for ns in (2, 3, 4):
            _split(ns)
            o, _ = _twice(dev, q, k, v, f"split ns{ns} dominant key")
            G._gate(o, q, k, v, f"split ns{ns} dominant key", ref=ref)
            for i, j in pairs:
                assert torch.equal(o[:, i].view(torch.int16), v[:, j].view(torch.int16)), f"ns{ns}: query {i} is not V row {j}"
    finally:
        G._clear()


def test_split_form_on_near_one_hot_rows(dev):
    shape = (1, 129, 193, 3)
    q, k, v = A.sharp_qkv(*shape, seed=11)
    ref = R.reference(q, k, v, SCALE)
    try:
        for ns in (2, 3, 4):
            _split(ns)
            o, _ = _twice(dev, q, k, v, f"split ns{ns} near-one-hot")
            G._gate(o, q, k, v, f"split ns{ns} near-one-hot", ref=ref)
    finally:
        G._clear()


@pytest.mark.parametrize("lazy", [0.0, 8.0, 12.0])
def test_split_form_with_a_creeping_maximum(dev, lazy):
    """1000 keys: 8 + 8 tiles, each range with a stale maximum of its own and the ragged tile in the second."""
    q, k, v = A.creeping_qkv()
    ref = R.reference(q, k, v, SCALE, lazy)
    try:
        for ns in (2, 3, 4):
            _split(ns, lazy=lazy)
            o, _ = _twice(dev, q, k, v, f"split ns{ns} creeping maximum, lazy {lazy}")
            G._gate(o, q, k, v, f"split ns{ns} creeping maximum, lazy {lazy}", lazy=lazy, ref=ref)
    finally:
        G._clear()


def test_default_dispatch_follows_the_plan(dev):
    """No override: the form ctx_attention_plan reports for the device's CU count is the one that runs: the launch matches the forced
    launch of that form bit for bit (the forms differ in their bits: the 4- and 8-wave ones in nothing but the split one in its
    merge; which shapes the model gives to which form is tests/test_attention_split_cpu.py's matter)."""
    import ctypes as C
    L, lib = G._lib()
    G._clear()
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    out = (C.c_int32 * 4)()
    for shape in [(2, 1152, 1152, 2), (1, 257, 320, 3)]:
        L.check(lib.ctx_attention_plan(*shape, n_cu, C.cast(out, C.c_void_p)))
        q, k, v = A.random_qkv(*shape, A.case_seed(*shape))
        o, _ = G._launch(dev, q, k, v)
        try:
            lib.ctx_attention_tune(-1, {4: 0, 8: 1, 12: 2}[out[0]], -1, -1.0)
            forced, _ = G._launch(dev, q, k, v)
        finally:
            G._clear()
        print(f"{shape} on {n_cu} CUs: plan {list(out)}")
        assert torch.equal(o.view(torch.int16), forced.view(torch.int16))
        G._gate(o, q, k, v, f"default dispatch {shape}", ref=R.reference(q, k, v, SCALE) if out[1] == 2 else None)
