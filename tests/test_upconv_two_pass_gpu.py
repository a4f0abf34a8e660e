"""upconv_gather_kernel's two-pass form (csrc/upconv.hip): per source row one horizontal pass into a ring of Hrow rows,
per output row one vertical pass over that ring, the z rows a band adds staged in chunks.  Shapes where a ring, a chunk
or the image-to-workgroup mapping can go wrong, held like test_conv3x3_upsampled_vs_fp64 (tests/test_net_gpu.py): the
two TF-1.8 operators of oracle/net.py in float64 at <= 1e-5 of the tensor scale, the library's own resize + conv2d at
the same bound, and bit-equal when run again.

Both output layouts: NHWC through mpsr_conv3x3_upsampled_f32, channel-blocked through the decoder entry point (there
the gather writes [C/8][H][W][8] for the F(4x4,3x3) layer that follows).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import net as onet

pytestmark = pytest.mark.gpu

C_IN, N_OUT = 128, 128  # the narrowest layer the tap GEMM takes: 16 channel blocks per image

CASES = {
    # name: (B, h, w, OH, OW, align_corners)
    "nine_images": (9, 3, 5, 6, 10, True),        # a partly filled group of 8 images: image -> workgroup mapping
    "bands_ragged": (2, 14, 14, 27, 27, True),    # four bands, the last of 3 rows: band roll-over, the ring wraps
    "bands_legacy": (2, 14, 14, 27, 27, False),   # the same with the legacy scale: source rows clamp at the bottom
    "one_and_a_half": (2, 8, 8, 12, 12, True),    # 1.5x: uneven tap weights
    "identity": (2, 12, 12, 12, 12, True),        # h = H: every tap hits one source row; two chunks of staged rows
    "half_legacy": (9, 3, 5, 6, 10, False),       # scale exactly 1/2: every bilinear weight is 0, 1/2 or 1
    "wide_rows": (2, 3, 70, 4, 136, True),        # a z row wider than the prefetch registers: one row per chunk, in rounds
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize("name", ["nine_images", "bands_ragged", "bands_legacy", "one_and_a_half", "identity",
                                  "wide_rows"])
@pytest.mark.parametrize("has_bias,relu", [(True, True), (False, False)])
def test_two_pass_gather_vs_fp64(name, has_bias, relu):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    B, h, w, OH, OW, align = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + int(relu))
    x = rng.standard_normal((B, h, w, C_IN)).astype(np.float32)
    wgt = (rng.standard_normal((3, 3, C_IN, N_OUT)) / np.sqrt(9 * C_IN)).astype(np.float32)
    bias = rng.standard_normal(N_OUT).astype(np.float32) if has_bias else None
    up = onet.tf_resize_bilinear(torch.from_numpy(x).double(), OH, OW, align)
    ref = onet.tf_conv2d(up, torch.from_numpy(wgt).double())
    if has_bias:
        ref = ref + torch.from_numpy(bias).double()
    if relu:
        ref = torch.relu(ref)
    w_ok, _ = W.fold_conv(wgt)
    args = (_dev(x), (OH, OW), _dev(w_ok), _dev(bias) if has_bias else None, relu, align)
    got = dn.conv3x3_upsampled(*args)
    again = dn.conv3x3_upsampled(*args)
    e64 = _err(got, ref)
    two = dn.conv2d(dn.resize_bilinear(_dev(x), (OH, OW), align), _dev(w_ok), _dev(bias) if has_bias else None, None, 3,
                    3, 1, relu)
    e32 = _err(got, two)
    print("%s: vs fp64 %.3e, vs resize + conv2d %.3e" % (name, e64, e32))
    assert e64 <= 1e-5, "%s vs fp64: %.3e" % (name, e64)
    assert e32 <= 1e-5, "%s vs resize + conv2d: %.3e" % (name, e32)
    assert torch.equal(got, again), "not deterministic"


@pytest.mark.parametrize("name", ["identity", "half_legacy"])
def test_all_ones_count_the_taps_exactly(name):
    """Inputs 1, every filter tap 1 on one input channel and 0 on the others, no bias: an output is the number of
    taps inside the upsampled image -- 9 inside, 6 on an edge, 4 in a corner -- EXACTLY on the
    two cases whose bilinear weights are 0, 1/2 or 1 (identity scale; legacy scale 1/2): every product and partial sum
    of both passes is then a small multiple of 1/4 and no rounding happens.  (At other scales the weight pairs
    (1 - l, l) are rounded and a sum of nine such pairs need not round to 9; those scales are held to float64 above.)"""
    from monopsr_amd.core import device_net as dn
    B, h, w, OH, OW, align = CASES[name]
    x = torch.ones((B, h, w, C_IN), device="cuda")
    w_ok = torch.zeros((N_OUT, 9, C_IN), device="cuda")
    w_ok[:, :, 0] = 1.0  # one input channel carries the 1: the tap GEMM's z is exactly 1 for every tap
    got = dn.conv3x3_upsampled(x, (OH, OW), w_ok.reshape(N_OUT, 9 * C_IN), None, False, align)
    ny = torch.full((OH,), 3.0)
    nx = torch.full((OW,), 3.0)
    ny[0] = ny[-1] = 2.0
    nx[0] = nx[-1] = 2.0
    want = (ny[:, None] * nx[None, :])[None, :, :, None].expand(B, OH, OW, N_OUT)
    assert torch.equal(got.cpu(), want), "largest difference %.3e" % float((got.cpu() - want).abs().max())
    assert float(got[0, 1, 1, 0]) == 9.0 and float(got[0, 0, 1, 0]) == 6.0 and float(got[0, 0, 0, 0]) == 4.0


def _decoder_net(width_div, seed):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    weights = W.synthetic_weights(seed=seed, width_div=width_div, trunk=False, heads=False)
    net = dn.DeviceNet.__new__(dn.DeviceNet)
    net.device = torch.device("cuda")
    net.decoder = dn.PackedPart(*W.pack_decoder(weights, width_div), net.device)
    net.ws_dec = dn.Workspace(net.device)
    return net


def _decoder_both_ways(net, crop, full):
    from monopsr_amd import _lib
    lib = _lib.lib()
    outs = {}
    for on in (1, 0):
        lib.mpsr_debug_set_decoder_upconv(on)
        try:
            net.fcache = {}
            outs[on] = [t.clone() for t in net.squash_decoder(crop, full, (48, 48), want_feat_map=True)]
            if on:
                again = net.squash_decoder(crop, full, (48, 48), want_feat_map=True)
                for a, b in zip(outs[on], again):
                    assert torch.equal(a, b), "not deterministic"
        finally:
            lib.mpsr_debug_set_decoder_upconv(1)
    return outs


def _decoder_kinds(net, B):
    from monopsr_amd import _lib
    kinds = (ctypes.c_int * 7)()
    flops = (ctypes.c_double * 7)()
    _lib.check(_lib.lib().mpsr_squash_decoder_plan(B, 12, 12, 48, 48, net.decoder.layers, net.decoder.n, kinds, flops))
    return tuple(kinds)


@pytest.mark.parametrize("width_div,B,chain", [(4, 3, None), (1, 117, (7, 3, 7, 3))])
def test_decoder_with_the_gather_vs_resize_chain(width_div, B, chain):
    """The whole decoder with conv2_1 / conv3_1 as tap GEMM + gather against mpsr_debug_set_decoder_upconv(0) (resize +
    conv), at the bound test_decoder_upsampled_convs_as_tap_gemm_vs_resize_winograd holds: 1e-4 of each output's scale.
    width_div 4, B = 3: the small-batch chain.  Full width, B = 117 (117 * 24 * 24 >= 65536, a partly filled group of 8
    images): the channel-blocked chain, where both gathers (one band at 12 -> 24, six bands at 24 -> 48) write
    [C/8][H][W][8] for the F(4x4,3x3) layer behind them -- the plan says so."""
    net = _decoder_net(width_div, seed=31 + width_div)
    if chain is not None:
        assert _decoder_kinds(net, B)[2:6] == chain
    g = torch.Generator(device="cuda").manual_seed(17 + width_div)
    c = 1024 // width_div
    crop = torch.randn((B, 12, 12, c), device="cuda", generator=g).clamp_(min=0)
    full = torch.randn((B, 12, 12, c), device="cuda", generator=g).clamp_(min=0)
    outs = _decoder_both_ways(net, crop, full)
    for name, a, b in zip(("features_for_box_3d", "features_for_map", "inst_xyz_map_local"), outs[1], outs[0]):
        e = _err(a, b)
        print("width_div %d %s: %.3e" % (width_div, name, e))
        assert e < 1e-4, (name, e)
    assert float(outs[1][2].abs().max()) > 0
