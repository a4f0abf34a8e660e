"""Shapes of the trunk / decoder / heads sweeps off the 12 -> 24 -> 48 geometry (tests/test_net_shapes.py and
tests/test_net_shapes_gpu.py), the plans they are meant to reach and the small host-side helpers both files share.

Every shape below was chosen from the dispatchers' own predicates; the comments name the predicate a case trips.  The
plan (mpsr_squash_decoder_plan / mpsr_conv2d_plan) is asserted per case, so a retuned threshold shows up as a failed
plan assertion instead of a sweep that quietly stopped reaching its branch.
"""
import ctypes
import functools

import numpy as np

PLAN = None  # in a `kinds` tuple: "whatever mpsr_conv2d_plan says for this layer's shape"


class DecoderCase:
    def __init__(self, name, fh, fw, mh, mw, B, kinds, kinds_wd1=None, resize_only=False):
        self.name, self.fh, self.fw, self.mh, self.mw, self.B = name, fh, fw, mh, mw, B
        self.kinds = kinds            # layers 2..5 (conv2_1, conv2_2, conv3_1, conv3_2) at width_div = 2
        self.kinds_wd1 = kinds_wd1    # ... at full width, for the cases that also run there
        self.resize_only = resize_only  # also run with the tap GEMM disabled: both resizes + four F(4x4,3x3) layers

    def __repr__(self):
        return self.name

    @property
    def map_size(self):
        return (self.mh, self.mw)


# The decoder's governing predicate is conv2d_takes_winograd4 at the half-size map (hh, hw) = (mh / 2, mw / 2):
# hh % 4 == hw % 4 == 0, C, N >= 64 and B * hh * hw >= 65536.  All four 3x3 layers on F(4x4,3x3) or the tap GEMM
# (kinds 3 / 7) is the channel-blocked ("c8") chain; anything else is the NHWC chain.  At width_div = 2 the layers are
# 256 -> 128, 128 -> 128, 128 -> 64, 64 -> 64: only conv2_1 has the N % 128 == 0 the tap GEMM wants; at full width
# conv3_1 (256 -> 128) has it too.  Every B of D1 - D4 is the smallest that reaches the branch: one instance fewer and
# the plan falls back to the NHWC chain.
#
# What mpsr::resize_bilinear_c8 does (the plan cannot see it; it runs when a c8 chain's upsampled layer is NOT a tap
# GEMM, i.e. for conv3_1 at width_div = 2 and for both resizes under mpsr_debug_set_decoder_upconv(0)).  LDS kernel
# iff OW <= 128, the source rows of RO output rows fit kResizeLdsMaxRows = 16, and 16 source rows of W pixels fit 48 KiB
# (W <= 96); passes = 4 only from OH >= 40 on, so every LDS launch below runs ONE pass of 256 / OW output rows:
#   D1  8x8 -> 16x16 -> 32x32     LDS both times: OW = 16 (RO clipped to OH = 16, one row block), OW = 32 (8 rows, 4 blocks)
#   D2  6x20 -> 12x40 -> 24x80    LDS both times: 256 / 40 = 6 rows (16 idle threads), 256 / 80 = 3 rows (16 idle threads)
#   D3  3x70 -> 4x136 -> 8x272    OW = 136, 272 > 128: resize_bilinear_c8out_kernel (plain) both times
#   D4  10x100 -> 12x104 -> 24x208  first: OW = 104 <= 128 but W = 100 > 96 (LDS window 51200 B > 48 KiB): plain kernel;
#                                   second: OW = 208 > 128: plain kernel
DECODER_CASES = [
    # c8 chain at a non-48 square; B * hh * hw = 256 * 16 * 16 is exactly 65536 (the >= boundary).  Full width: two tap GEMMs.
    DecoderCase("D1", 8, 8, 32, 32, 256, (7, 3, 3, 3), kinds_wd1=(7, 3, 7, 3), resize_only=True),
    # c8 chain, non-square; 137 * 12 * 40 = 65760 (136: 65280).  Full width: upconv_applies refuses conv3_1 (the 12x40 ->
    # 24x80 gather does not fit gather_geometry, upconv.hip), so it stays one tap GEMM + one resize.
    DecoderCase("D2", 6, 20, 24, 80, 137, (7, 3, 3, 3), kinds_wd1=(7, 3, 3, 3), resize_only=True),
    # c8 chain with OW > 128; 121 * 4 * 136 = 65824 (120: 65280)
    DecoderCase("D3", 3, 70, 8, 272, 121, (7, 3, 3, 3), resize_only=True),
    # c8 chain with no tap GEMM by itself (upconv_applies refuses both layers: rows this wide do not fit gather_geometry,
    # upconv.hip); 53 * 12 * 104 = 66144 (52: 64896)
    DecoderCase("D4", 10, 100, 24, 208, 53, (3, 3, 3, 3), resize_only=True),
    # a map smaller than the features (hscale = 23 / 7 > 1 on the first resize), NHWC chain; no tap GEMM (downsampling)
    DecoderCase("D5", 24, 24, 16, 32, 2, (PLAN, PLAN, PLAN, PLAN)),
    # first resize is the identity (the oracle returns its input, the kernels run at scale 1); ragged NHWC chain
    DecoderCase("D6", 5, 7, 10, 14, 3, (7, PLAN, PLAN, PLAN)),
    # odd fh, fw: the VALID 2x2 pool drops a row and a column; odd half-size 13x9
    DecoderCase("D7", 7, 9, 26, 18, 2, (7, PLAN, PLAN, PLAN)),
    # smallest accepted call: resize to 1x1 (OH == 1: scale = in / out instead of (in-1) / (out-1)), 1x1 pool output
    DecoderCase("D8", 2, 2, 2, 2, 1, (7, PLAN, PLAN, PLAN)),
    # small-batch F(3x3,3x3)-tiles rule for dense layers (conv2d_takes_winograd3: H == W, H / 3 <= 16, >= 1024 tiles):
    # 18x18 and 36x36 qualify (kind 4) ...
    DecoderCase("D9a", 9, 9, 36, 36, 32, (7, 4, 4, 4)),
    # ... 48x48 does, 96x96 (32 tiles a side) does not -- and 8 * 96 * 96 >= 65536 pixels sends it to F(4x4,3x3)
    # inside the NHWC chain
    DecoderCase("D9b", 24, 24, 96, 96, 8, (7, 4, 3, 3)),
]
DECODER_BY_NAME = {c.name: c for c in DECODER_CASES}
RESIZE_ONLY_CASES = [c for c in DECODER_CASES if c.resize_only]
FULL_WIDTH_CASES = [c for c in DECODER_CASES if c.kinds_wd1 is not None]
HEADS_CASES = ["D2", "D7", "D8"]  # img_fc K = (fh//2) * (fw//2) * 256 = 7680, 3072, 256: both sides of the few-row FC
HEADS_BATCHES = [1, 137]          # kernel's 4096 limit, one at its 128 minimum region


# Trunk inputs (B, H, W) at width_div = 2 and the kinds mpsr_conv2d_plan gives block2's / block3's 3x3 layer (64 -> 64
# at dilation 2, 128 -> 128 at dilation 4) on the block3 map.  conv2d()'s rules: F(3x3,3x3) / sixteen products (kind 4)
# wants H == W, H % (3 d) == 0 and, unless a sub-grid is ONE 3x3 tile, >= 1024 tiles and at most 2 x 2 tiles per
# sub-grid; F(2x2) on sub-grids (kind 1) wants H % (2 d) == W % (2 d) == 0 and B * H * W >= 12000 pixels.  At one or
# two images none of the first five reaches a transform-domain kernel: the last three are the same geometries at the
# smallest size / batch where the rule fires.
TRUNK_CASES = [
    # B, H, W, (kind of block2 conv2, kind of block3 conv2), what it covers
    (2, 40, 56, (0, 0), "10x14: no sub-grid rule applies at dilation 2 or 4"),
    (1, 50, 46, (0, 0), "13x12: odd height"),
    (2, 96, 96, (0, 0), "24x24: 4 x 4 / 2 x 2 tiles per sub-grid, below the 1024 tiles of the tiled forms"),
    (1, 32, 64, (0, 0), "8x16: whole even sub-grids at dilation 4, below F(2x2)'s 12000 pixels"),
    (1, 7, 7, (0, 0), "2x2: smaller than the dilation, every non-centre tap of block3 is padding"),
    (94, 32, 64, (1, 1), "8x16 x 94 = 12032 pixels: F(2x2,3x3) on dilation-2 and dilation-4 sub-grids, non-square"),
    (16, 96, 96, (0, 4), "24x24 x 16: 2 x 2 tiles with halos per dilation-4 sub-grid (1024 tiles); 4 x 4 at dilation 2 never"),
    (3, 21, 23, (4, 0), "6x6 from odd input sizes: block2's sub-grids are single 3x3 tiles (sixteen products), block3's map is below 3 d"),
]


# oracle.net.tf_resize_bilinear(align_corners=True) in float64 against torch's bilinear interpolate on the decoder
# cases' resizes (every output dimension > 1): (h, w, OH, OW, measured gap).  The two differ only by TF's float32
# source coordinate; gap = max |tf - torch| / max |torch| on net_shape_cases.resize_input, measured on the host.
RESIZE_GAPS = [
    (8, 8, 16, 16, 3.2e-07), (16, 16, 32, 32, 1.1e-06), (6, 20, 12, 40, 7.7e-07), (12, 40, 24, 80, 2.4e-06),
    (3, 70, 4, 136, 5.2e-06), (4, 136, 8, 272, 7.0e-06), (10, 100, 12, 104, 7.1e-06), (12, 104, 24, 208, 7.0e-06),
    (24, 24, 8, 16, 1.2e-06), (8, 16, 16, 32, 6.4e-07), (5, 7, 5, 7, 0.0), (5, 7, 10, 14, 2.1e-07),
    (7, 9, 13, 9, 0.0), (13, 9, 26, 18, 8.0e-07), (1, 1, 2, 2, 0.0), (9, 9, 18, 18, 4.1e-07),
    (18, 18, 36, 36, 9.3e-07), (24, 24, 48, 48, 1.4e-06), (48, 48, 96, 96, 4.1e-06),
]


def resize_input(h, w):
    return np.random.default_rng(h * 1000 + w).standard_normal((2, h, w, 5))


def oracle_picks(B):
    """The instances a batch is held to the fp64 oracle on: all of a small batch; first, middle and last of a large one."""
    return list(range(B)) if B <= 3 else [0, B // 2, B - 1]


@functools.lru_cache(maxsize=None)
def decoder_layers(width_div):
    """The seven decoder layer records at a width (no weights: what the plans read)."""
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    recs = []
    for name, kh, kw, cin, cout, _, _, relu in W.scaled_decoder_specs(width_div):
        if name.startswith("squash"):
            recs.append(dict(cin=cin // 2, cout=cout, kh=1, kw=1, dilation=1, relu=0, w_off=0, b_off=-1))
            recs.append(dict(cin=cin // 2, cout=cout, kh=1, kw=1, dilation=1, relu=int(relu), w_off=0, b_off=0))
        else:
            recs.append(dict(cin=cin, cout=cout, kh=kh, kw=kw, dilation=1, relu=int(relu), w_off=0, b_off=0))
    return recs, dn._layer_array(recs)


def conv_kind(B, H, Wd, C, N, k, dilation):
    from monopsr_amd import _lib
    kind, ex = ctypes.c_int(-1), ctypes.c_double(0)
    _lib.check(_lib.lib().mpsr_conv2d_plan(B, H, Wd, C, N, k, k, dilation, ctypes.byref(kind), ctypes.byref(ex)))
    return kind.value


def decoder_plan(case, width_div, upconv=1):
    """-> (kinds of layers 2..5 as mpsr_squash_decoder_plan reports them, the same layers one by one through
    mpsr_conv2d_plan)."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    recs, layers = decoder_layers(width_div)
    kinds, ex = (ctypes.c_int * 7)(), (ctypes.c_double * 7)()
    lib.mpsr_debug_set_decoder_upconv(upconv)
    try:
        _lib.check(lib.mpsr_squash_decoder_plan(case.B, case.fh, case.fw, case.mh, case.mw, layers, 7, kinds, ex))
    finally:
        lib.mpsr_debug_set_decoder_upconv(1)
    hh, hw = case.mh // 2, case.mw // 2
    sizes = {2: (hh, hw), 3: (hh, hw), 4: (case.mh, case.mw), 5: (case.mh, case.mw)}
    single = tuple(conv_kind(case.B, sizes[i][0], sizes[i][1], recs[i]["cin"], recs[i]["cout"], 3, 1) for i in (2, 3, 4, 5))
    return tuple(kinds[2:6]), single


def chain_of(kinds):
    """Which chain mpsr_squash_decoder_fwd runs for the planned kinds of layers 2..5 (decoder_choice, network.hip): the
    c8 chain needs conv2_2 and conv3_2 on F(4x4,3x3) and each upsampled layer on F(4x4,3x3) or the tap GEMM."""
    if kinds[1] == 3 and kinds[3] == 3 and kinds[0] in (3, 7) and kinds[2] in (3, 7):
        return "c8, %d tap GEMM" % ((kinds[0] == 7) + (kinds[2] == 7))
    return "nhwc"


def check_decoder_plan(case, width_div, upconv=1):
    """Asserts the kinds the case was designed for and returns the chain."""
    want = (3, 3, 3, 3) if not upconv else (case.kinds if width_div == 2 else case.kinds_wd1)
    got, single = decoder_plan(case, width_div, upconv)
    for i, (w, g, s) in enumerate(zip(want, got, single)):
        assert g == (s if w is PLAN else w), "%s width_div %d layer %d: planned %s, single-layer plan %s, designed for %s" % (
            case.name, width_div, i + 2, got, single, want)
    return chain_of(got)


def trunk_map(H, Wd):
    oh, ow = (H - 1) // 2 + 1, (Wd - 1) // 2 + 1
    return (oh + 1) // 2, (ow + 1) // 2


def trunk_plan(B, H, Wd, width_div=2):
    ph, pw = trunk_map(H, Wd)
    return (conv_kind(B, ph, pw, 128 // width_div, 128 // width_div, 3, 2),
            conv_kind(B, ph, pw, 256 // width_div, 256 // width_div, 3, 4))


def head_inputs(B, seed):
    """Box scalars of the heads in KITTI's ranges."""
    rng = np.random.default_rng(seed)
    y1 = rng.uniform(0, 150, B)
    x1 = rng.uniform(0, 1000, B)
    boxes = np.stack([y1, x1, y1 + rng.uniform(20, 200, B), x1 + rng.uniform(20, 200, B)], 1).astype(np.float32)
    cam_p = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
                      [0.0, 0.0, 1.0, 0.002745884]], np.float32)  # a KITTI P2
    view = rng.uniform(-0.6, 0.6, B).astype(np.float32)
    cls = np.ones((B, 1), np.int32)
    mean_lwh = np.tile(np.array([[3.88, 1.63, 1.53]], np.float32), (B, 1))
    z_off = np.full((B,), 2.17799973487854, np.float32)
    return boxes, cam_p, view, cls, mean_lwh, z_off
