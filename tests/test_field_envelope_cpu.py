"""CPU: the host gate of the texture-field MLP (csrc/uvmlp.hip) through its three size queries, which launch nothing.

The envelope is stated once below as a plain predicate written from the text of include/ctx_nerf.h ("The envelope of every
ctx_uvmlp_* entry point"); nothing here is imported from the library.  Every query must answer >= 0 exactly on it and -1 elsewhere
(W = 192, a multiple of 64 the kernels have no form for, is the case that used to be accepted), and the byte counts must follow the
closed forms the header gives."""
import itertools

import pytest

DS = (0, 1, 2, 8, 16, 17)
WS = (0, 32, 64, 96, 128, 192, 256, 320, 512)
INS = (0, 1, 47, 48, 49, 64, 65)
OUTS = (0, 1, 4, 5)
NS = (-1, 0, 1, 64, 65, 193)


def in_envelope(D, W, input_ch=1, output_ch=1):
    """include/ctx_nerf.h: 1 <= D <= 16, W in {64, 128, 256}, 1 <= input_ch <= 64, 1 <= output_ch <= 4 (any skip)."""
    return 1 <= D <= 16 and W in (64, 128, 256) and 1 <= input_ch <= 64 and 1 <= output_ch <= 4


def skips_of(D):
    """skip is never a reason to refuse a size: inside [0, D-2] it names the skip layer, outside it means none."""
    return sorted({-1, 0, 4, D - 2, D - 1, 99})


def n_params(D, W, input_ch, output_ch, skip):
    """the nn.Linear parameters of NeRF2D(D, W, input_ch, output_ch, skips=[skip]) (weights and biases)."""
    n = input_ch * W + W
    for i in range(1, D):
        n += (W + (input_ch if i == skip + 1 else 0)) * W + W
    return n + output_ch * W + output_ch


@pytest.fixture(scope="module")
def lib():
    from contexture_nerf_amd import _lib as L
    return L.load()


def test_packed_bytes_envelope_and_floor(lib):
    n_in = n_out = 0
    for D, W, ic, oc in itertools.product(DS, WS, INS, OUTS):
        for skip in skips_of(D):
            b = lib.ctx_uvmlp_packed_bytes(D, W, ic, oc, skip)
            if in_envelope(D, W, ic, oc):
                n_in += 1
                assert b >= 4 * n_params(D, W, ic, oc, skip), (D, W, ic, oc, skip, b)
                assert b % 4 == 0
            else:
                n_out += 1
                assert b == -1, (D, W, ic, oc, skip, b)
    assert n_in > 500 and n_out > 5000                    # the sweep really has both sides


@pytest.mark.parametrize("W", [64, 128, 256])
def test_packed_bytes_monotone_in_depth(lib, W):
    for ic, oc, skip in itertools.product((1, 47, 48, 49, 64), (1, 4), (-1, 0, 4, 99)):
        sizes = [lib.ctx_uvmlp_packed_bytes(D, W, ic, oc, skip) for D in range(1, 17)]
        assert all(a > 0 for a in sizes)
        assert all(b > a for a, b in zip(sizes, sizes[1:])), (W, ic, oc, skip, sizes)     # a layer more is at least its W x W weights more
        assert lib.ctx_uvmlp_packed_bytes(17, W, ic, oc, skip) == -1


def test_saved_bytes_envelope_and_closed_form(lib):
    for N, D, W, ic in itertools.product(NS, DS, WS, INS):
        b = lib.ctx_uvmlp_saved_bytes(N, D, W, ic)
        if N >= 1 and in_envelope(D, W, ic):
            EP = 48 if ic <= 48 else 64
            assert b == N * (EP + D * W) * 4 + D * -(-N // 64) * W * 8, (N, D, W, ic, b)
        else:
            assert b == -1, (N, D, W, ic, b)


def test_bwd_ws_bytes_envelope(lib):
    for N, D, W in itertools.product(NS, DS, WS):
        b = lib.ctx_uvmlp_bwd_ws_bytes(N, D, W)
        if N >= 1 and in_envelope(D, W):
            assert b >= D * N * W * 4 and b % 256 == 0, (N, D, W, b)        # at least the dZ rows [D, N, W] it is documented to hold
        else:
            assert b == -1, (N, D, W, b)
    # it grows with the texel count and the depth (the dZ rows do)
    for W in (64, 128, 256):
        assert lib.ctx_uvmlp_bwd_ws_bytes(193, 8, W) > lib.ctx_uvmlp_bwd_ws_bytes(65, 8, W) > lib.ctx_uvmlp_bwd_ws_bytes(1, 8, W)
        assert lib.ctx_uvmlp_bwd_ws_bytes(193, 16, W) > lib.ctx_uvmlp_bwd_ws_bytes(193, 8, W)


def test_width_192_is_refused_everywhere_a_size_is_asked(lib):
    """the shape that was accepted and then run through the W = 64 kernels"""
    assert lib.ctx_uvmlp_packed_bytes(8, 192, 42, 3, 4) == -1
    assert lib.ctx_uvmlp_saved_bytes(4096, 8, 192, 42) == -1
    assert lib.ctx_uvmlp_bwd_ws_bytes(4096, 8, 192) == -1
    for W in (64, 128, 256):
        assert lib.ctx_uvmlp_packed_bytes(8, W, 42, 3, 4) > 0
