"""Host-side half of the network shape sweep (tests/net_shape_cases.py; the GPU half is tests/test_net_shapes_gpu.py):
the oracle itself away from 48x48, and the plans -- which kernels the dispatchers pick for every case of the sweep.  The
plan functions are host code of libmonopsr_hip.so and need no GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net_shape_cases as C
from oracle import net as onet


@pytest.mark.parametrize("h,w,OH,OW,measured", C.RESIZE_GAPS, ids=["%dx%d-%dx%d" % g[:4] for g in C.RESIZE_GAPS])
def test_oracle_resize_against_torch_interpolate(h, w, OH, OW, measured):
    """tf_resize_bilinear(align_corners=True) in float64 at the decoder cases' sizes against torch's bilinear
    interpolate.  The only difference is the float32 source coordinate TF computes (a relative 2^-24 on a coordinate of
    up to 136 moves a sample by ~1e-5 of a pixel): the gap measured per size is in net_shape_cases.RESIZE_GAPS (largest:
    7.1e-6 of the tensor's scale at 10x100 -> 12x104) and is asserted with a 2x margin; the sizes whose scale is
    exact in float32 (identity, 0.5, 0) agree to float64 rounding."""
    x = torch.from_numpy(C.resize_input(h, w))
    got = onet.tf_resize_bilinear(x, OH, OW, True)
    ref = F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, OH, OW, 5)
    gap = float((got - ref).abs().max() / ref.abs().max())
    print("resize %dx%d -> %dx%d: gap %.3e (measured %.1e)" % (h, w, OH, OW, gap, measured))
    assert gap <= max(2 * measured, 1e-14)


def test_resize_gap_table_covers_every_decoder_case():
    """Both resizes of every decoder case with all output dimensions > 1 are in the table (D8's 2x2 -> 1x1 is not)."""
    have = {g[:4] for g in C.RESIZE_GAPS}
    for c in C.DECODER_CASES:
        hh, hw = c.mh // 2, c.mw // 2
        for step in ((c.fh, c.fw, hh, hw), (hh, hw, c.mh, c.mw)):
            assert step in have or min(step[2:]) == 1, (c.name, step)


@pytest.mark.parametrize("name", ["D5", "D6", "D7", "D8"])
def test_oracle_squash_decoder_shapes(name):
    """Output shapes of the oracle's squash + decoder where the map is smaller than the features, equal to them, odd,
    and 2x2 (a narrow copy of the graph: shapes do not depend on the width)."""
    from monopsr_amd.core import weights as W
    c = C.DECODER_BY_NAME[name]
    wd = 16
    weights = W.synthetic_weights(seed=1, width_div=wd, trunk=False, heads=False)
    rng = np.random.default_rng(2)
    crop = torch.from_numpy(np.maximum(rng.standard_normal((c.B, c.fh, c.fw, 1024 // wd)), 0))
    full = torch.from_numpy(np.maximum(rng.standard_normal((c.B, c.fh, c.fw, 1024 // wd)), 0))
    fb, fm, xyz = onet.squash_decoder(crop, full, weights, c.mh, c.mw)
    assert tuple(fb.shape) == (c.B, c.fh // 2, c.fw // 2, 512 // wd)
    assert tuple(fm.shape) == (c.B, c.mh, c.mw, 128 // wd)
    assert tuple(xyz.shape) == (c.B, c.mh, c.mw, 3)
    assert fb.dtype == fm.dtype == xyz.dtype == torch.float64
    assert bool(torch.isfinite(xyz).all()) and float(xyz.abs().max()) > 0


def test_decoder_sweep_reaches_every_chain():
    """Every case plans the kinds it was designed for (7 = tap GEMM, 3 = F(4x4,3x3), otherwise mpsr_conv2d_plan's
    answer), and over the sweep each chain of mpsr_squash_decoder_fwd occurs: c8 with both resizes, c8 with one tap
    GEMM and one resize, c8 with two tap GEMMs, NHWC.  One instance fewer and D1 - D4 fall back to the NHWC chain: their
    B is the smallest that reaches the branch."""
    chains = set()
    for c in C.DECODER_CASES:
        chains.add(C.check_decoder_plan(c, 2))
        if c.kinds_wd1 is not None:
            chains.add(C.check_decoder_plan(c, 1))
        if c.resize_only:
            chains.add(C.check_decoder_plan(c, 2, upconv=0))
            smaller = C.DecoderCase(c.name, c.fh, c.fw, c.mh, c.mw, c.B - 1, c.kinds)
            assert C.chain_of(C.decoder_plan(smaller, 2)[0]) == "nhwc", c.name
    assert chains == {"c8, 0 tap GEMM", "c8, 1 tap GEMM", "c8, 2 tap GEMM", "nhwc"}, chains
    # by itself (no switch) the sweep reaches the resize-only c8 chain too: D4
    assert C.check_decoder_plan(C.DECODER_BY_NAME["D4"], 2) == "c8, 0 tap GEMM"


def test_trunk_sweep_reaches_every_3x3_kind():
    """Implicit GEMM (0), F(2x2,3x3) on atrous sub-grids (1) and the F(3x3,3x3) / sixteen-product forms (4) each serve
    a block2 / block3 3x3 layer somewhere in the trunk sweep."""
    seen = set()
    for B, H, Wd, kinds, what in C.TRUNK_CASES:
        assert C.trunk_plan(B, H, Wd) == kinds, what
        seen.update(kinds)
    assert {0, 1, 4} <= seen, seen
