"""The composite entry points -- mpsr_trunk_fwd_ex, mpsr_squash_decoder_fwd_ex, mpsr_heads_fwd_cams -- OFF the 12 -> 24
-> 48 geometry of the benchmark: every chain the dispatchers choose by shape and batch (tests/net_shape_cases.py names
the predicate behind each case), against the fp64 CPU restatement oracle/net.py on the same seeded inputs and weights.

Tolerance: the standing bound of the network path, max |got - ref| / max |ref| <= 1e-4 per output tensor
(tests/test_net_gpu.py).  Where the code claims bit identity -- the channel-blocked ("c8") chain against the NHWC chain on
the same kernels (network.hip), and with it the LDS / plain channel-blocked resize kernels against the NHWC resize
(image_ops.hip: "same taps, same arithmetic") -- the assertion is torch.equal.

Oracle cost.  BatchNorm is folded, instances are independent: a large batch is held to the oracle on its first, middle
and last instance, and as a whole to the same call under winograd_policy="off" with the c8 chain disabled (the direct
NHWC chain, itself held to the oracle on the three instances).

Every decoder call runs on a workspace of exactly mpsr_decoder_workspace_bytes bytes filled with NaN, and writes into
outputs whose memory held NaN: a slot that is too small, a row that is read before it is written or an output element
that is never stored shows up as a NaN, not as a stale correct value.
"""
import numpy as np
import pytest
import torch

import net_shape_cases as C
from oracle import net as onet

pytestmark = pytest.mark.gpu

TOL = 1e-4
OUTPUTS = ("features_for_box_3d", "features_for_map", "inst_xyz_map_local")
HEAD_KEYS = ("lwh", "lwh_offs", "alpha_bins", "alpha_regs", "prop_cen_z", "cen_y", "cen_y_offs", "cen_z", "cen_z_offs",
             "cen_x", "centroids", "view_ang")


def _err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu() if isinstance(ref, torch.Tensor) else torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))  # (a NaN anywhere gives NaN, which fails <=)


def _close(got, ref, what):
    err = _err(got, ref)
    print("%-70s %.3e" % (what, err))
    assert err <= TOL, "%s: max err / scale = %.3e" % (what, err)
    return err


# ------------------------------------------------------------------------------------------------ decoder

@pytest.fixture(scope="module")
def nets():
    """One DeviceNet per width for the whole sweep: its filter cache meets every geometry and every kernel choice in
    turn (the tags per layer must re-fill a slice that holds another form)."""
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    made = {}

    def get(width_div):
        if width_div not in made:
            weights = W.synthetic_weights(seed=21 + width_div, width_div=width_div, trunk=False, heads=False)
            net = dn.DeviceNet.__new__(dn.DeviceNet)
            net.device = torch.device("cuda")
            net.decoder = dn.PackedPart(*W.pack_decoder(weights, width_div), net.device)
            made[width_div] = (weights, net)
        return made[width_div]
    return get


def _features(case, width_div, B=None):
    g = torch.Generator(device="cuda").manual_seed(1000 * case.fh + case.fw + width_div)
    shape = (B or case.B, case.fh, case.fw, 1024 // width_div)
    return (torch.randn(shape, device="cuda", generator=g).clamp_(min=0),
            torch.randn(shape, device="cuda", generator=g).clamp_(min=0))


_ORACLE = {}


def _oracle(case, width_div, weights, crop, full):
    """fp64 oracle on the case's picked instances, computed once per (case, width)."""
    key = (case.name, width_div)
    if key not in _ORACLE:
        pick = C.oracle_picks(case.B)
        with torch.no_grad():
            _ORACLE[key] = onet.squash_decoder(crop[pick].cpu().double(), full[pick].cpu().double(), weights, case.mh,
                                               case.mw)
    return _ORACLE[key]


def _run(net, case, crop, full, want_feat_map, policy=None, c8=1, upconv=1):
    from monopsr_amd import _lib
    from monopsr_amd.core import device_net as dn
    lib = _lib.lib()
    B = crop.shape[0]
    recs = net.decoder.records
    # exactly the bytes the library asks for, poisoned; and NaN in the memory the outputs will be allocated from
    net.ws_dec = dn.Workspace(net.device)
    net.ws_dec.get(lib.mpsr_decoder_workspace_bytes(B, case.fh, case.fw, case.mh, case.mw)).fill_(0xFF)
    shapes = [(B, case.fh // 2, case.fw // 2, recs[1]["cout"]), (B, case.mh, case.mw, recs[6]["cout"])]
    if want_feat_map:
        shapes.insert(1, (B, case.mh, case.mw, recs[5]["cout"]))
    poison = [torch.full(s, float("nan"), device=net.device) for s in shapes]
    del poison
    lib.mpsr_debug_set_decoder_c8(c8)
    lib.mpsr_debug_set_decoder_upconv(upconv)
    net.winograd_policy = policy
    try:
        return net.squash_decoder(crop, full, case.map_size, want_feat_map=want_feat_map)
    finally:
        net.winograd_policy = None
        lib.mpsr_debug_set_decoder_upconv(1)
        lib.mpsr_debug_set_decoder_c8(1)


def _hold_to_references(tag, outs, direct, ref, pick):
    """outs of one call: the picked instances against the oracle, the whole batch against the direct chain."""
    idx = torch.as_tensor(pick, device="cuda")
    for name, got, d, r in zip(OUTPUTS, outs, direct, ref):
        if got is None:
            continue
        _close(got[idx], r, "%s %s vs fp64 oracle (instances %s)" % (tag, name, pick))
        if len(pick) < got.shape[0]:
            _close(got, d, "%s %s vs direct NHWC chain (whole batch)" % (tag, name))


def _direct_chain(net, case, crop, full, ref, pick, tag):
    direct = _run(net, case, crop, full, True, policy="off", c8=0)
    idx = torch.as_tensor(pick, device="cuda")
    for name, d, r in zip(OUTPUTS, direct, ref):
        _close(d[idx], r, "%s direct NHWC chain %s vs fp64 oracle" % (tag, name))
    return direct


DECODER_RUNS = [(c, 2) for c in C.DECODER_CASES] + [(c, 1) for c in C.FULL_WIDTH_CASES]


@pytest.mark.parametrize("case,width_div", DECODER_RUNS, ids=["%s-w%d" % (c.name, w) for c, w in DECODER_RUNS])
def test_decoder_geometry_vs_oracle(case, width_div, nets):
    """mpsr_squash_decoder_fwd_ex as the library dispatches it at each geometry of the sweep, with the feature map
    requested and without (only then may the xyz head read channel-blocked): plan as designed, all three outputs
    within 1e-4 of the oracle, repeated call (valid filter cache) bit-identical."""
    weights, net = nets(width_div)
    tag = "%s w%d" % (case.name, width_div)
    chain = C.check_decoder_plan(case, width_div)
    print("%s: %dx%d -> %dx%d, B = %d: %s" % (tag, case.fh, case.fw, case.mh, case.mw, case.B, chain))
    crop, full = _features(case, width_div)
    pick = C.oracle_picks(case.B)
    ref = _oracle(case, width_div, weights, crop, full)
    direct = _direct_chain(net, case, crop, full, ref, pick, tag)
    for want_feat_map in (True, False):
        outs = _run(net, case, crop, full, want_feat_map)
        assert (outs[1] is None) == (not want_feat_map)
        _hold_to_references("%s feat_map=%d" % (tag, want_feat_map), outs, direct, ref, pick)
        again = _run(net, case, crop, full, want_feat_map)
        for name, a, b in zip(OUTPUTS, outs, again):
            assert a is None or torch.equal(a, b), "%s %s: second call differs" % (tag, name)
    assert float(outs[2].abs().max()) > 0


@pytest.mark.parametrize("case", C.RESIZE_ONLY_CASES, ids=repr)
def test_decoder_resize_chain_vs_oracle_and_bit_identical_layouts(case, nets):
    """D1 - D4 with the tap GEMM disabled: both upsamplings through mpsr::resize_bilinear_c8 (LDS kernel for D1 / D2,
    plain channel-blocked kernel for D3 / D4) and all four 3x3 layers on F(4x4,3x3).  Within 1e-4 of the oracle, and
    the c8 chain equals the NHWC chain (resize_bilinear_rows_kernel + the same F(4x4,3x3) launches) bit for bit."""
    weights, net = nets(2)
    tag = "%s w2 resize-only" % case.name
    assert C.check_decoder_plan(case, 2, upconv=0) == "c8, 0 tap GEMM"
    crop, full = _features(case, 2)
    pick = C.oracle_picks(case.B)
    ref = _oracle(case, 2, weights, crop, full)
    direct = _direct_chain(net, case, crop, full, ref, pick, tag)
    for want_feat_map in (True, False):
        blocked = _run(net, case, crop, full, want_feat_map, upconv=0, c8=1)
        nhwc = _run(net, case, crop, full, want_feat_map, upconv=0, c8=0)
        _hold_to_references("%s feat_map=%d" % (tag, want_feat_map), blocked, direct, ref, pick)
        for name, a, b in zip(OUTPUTS, blocked, nhwc):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(a, b), "%s %s: c8 chain differs from the NHWC chain" % (tag, name)
    assert float(blocked[2].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ heads

@pytest.mark.parametrize("B", C.HEADS_BATCHES)
@pytest.mark.parametrize("name", C.HEADS_CASES)
def test_heads_at_other_feature_sizes_vs_oracle(name, B):
    """mpsr_heads_fwd_cams on the decoder's own features_for_box_3d at D2 / D7 / D8: img_fc K = 7680, 3072, 256 (the
    few-row FC kernel's limit is 4096, its minimum region 128), one row and 137.  The features are held to the oracle's
    squash + pool on the picked instances; every head output to oracle.net.heads on those same features."""
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    case = C.DECODER_BY_NAME[name]
    csq = 256
    feat_elems = (case.fh // 2) * (case.fw // 2) * csq
    weights = W.synthetic_weights(seed=31, width_div=2, trunk=False, feat_elems=feat_elems)
    net = dn.DeviceNet.__new__(dn.DeviceNet)
    net.device = torch.device("cuda")
    net.decoder = dn.PackedPart(*W.pack_decoder(weights, 2), net.device)
    net.heads = dn.PackedPart(*W.pack_heads(weights, feat_elems), net.device)
    net.ws_dec, net.ws_heads = dn.Workspace(net.device), dn.Workspace(net.device)
    crop, full = _features(case, 2, B)
    feat = net.squash_decoder(crop, full, case.map_size, want_feat_map=False)[0]
    assert tuple(feat.shape) == (B, case.fh // 2, case.fw // 2, csq) and feat[0].numel() == feat_elems
    pick = C.oracle_picks(B)
    with torch.no_grad():
        x = torch.cat([crop[pick].cpu().double(), full[pick].cpu().double()], dim=3)
        sq = torch.relu(onet.tf_conv2d(x, torch.from_numpy(weights["squash/1x1_conv/weights"]).double()) +
                        torch.from_numpy(weights["squash/1x1_conv/biases"]).double())
        _close(feat[torch.as_tensor(pick, device="cuda")], onet.tf_max_pool(sq, 2, 2, "VALID"),
               "%s B=%d features_for_box_3d" % (name, B))
        boxes, cam_p, view, cls, mean_lwh, z_off = C.head_inputs(B, 7 + B)
        ref = onet.heads(feat.cpu().double(), boxes, cam_p, view, cls, mean_lwh, z_off, weights)
    dev = lambda a: torch.from_numpy(a).cuda()
    got = net.heads_fwd(feat, dev(boxes), dev(cam_p), dev(view), dev(cls), dev(mean_lwh), dev(z_off))
    for key in HEAD_KEYS:
        _close(got[key], ref[key], "%s B=%d K=%d %s" % (name, B, feat_elems, key))


# ------------------------------------------------------------------------------------------------ trunk

@pytest.fixture(scope="module")
def trunk_net():
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    weights = W.synthetic_weights(seed=41, width_div=2, decoder=False, heads=False)
    net = dn.DeviceNet.__new__(dn.DeviceNet)
    net.device = torch.device("cuda")
    net.crop_trunk = dn.PackedPart(*W.pack_trunk(weights, W.CROP_SCOPE, 2), net.device)
    net.full_trunk = None
    net.ws_trunk = dn.Workspace(net.device)
    return weights, net


@pytest.mark.parametrize("B,H,Wd,kinds,what", C.TRUNK_CASES, ids=["%dx%dx%d" % c[:3] for c in C.TRUNK_CASES])
def test_trunk_geometry_vs_oracle(B, H, Wd, kinds, what, trunk_net):
    """mpsr_trunk_fwd_ex at width_div = 2 on inputs other than 48x48 crops and the 160x608 image, against
    oracle.net.resnet101_block3 in fp64: the kinds conv2d() picks for block2's / block3's 3x3 layers are the ones the
    case was chosen for; a large batch is held to the oracle on three instances and as a whole to
    winograd_policy="off"."""
    from monopsr_amd.core import weights as W
    weights, net = trunk_net
    assert C.trunk_plan(B, H, Wd) == kinds, what
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + Wd)
    img = torch.randn((B, H, Wd, 3), device="cuda", generator=g) * 50
    pick = C.oracle_picks(B)
    with torch.no_grad():
        ref = onet.resnet101_block3(img[pick].cpu().double(), weights, W.CROP_SCOPE)
    net.ws_trunk = type(net.ws_trunk)(net.device)
    got = net.trunk(img)
    ph, pw = C.trunk_map(H, Wd)
    assert tuple(got.shape) == (B, ph, pw, 512)
    tag = "trunk (%d,%d,%d) -> %dx%d" % (B, H, Wd, ph, pw)
    _close(got[torch.as_tensor(pick, device="cuda")], ref, "%s block3 vs fp64 oracle (instances %s)" % (tag, pick))
    assert torch.equal(got, net.trunk(img)), "%s: second call (valid filter cache) differs" % tag
    if len(pick) < B:
        net.winograd_policy = "off"
        try:
            direct = net.trunk(img)
        finally:
            net.winograd_policy = None
        _close(direct[torch.as_tensor(pick, device="cuda")], ref, "%s direct chain vs fp64 oracle" % tag)
        _close(got, direct, "%s vs direct chain (whole batch)" % tag)
