"""How a layer's transformed filters travel between the network entry points and the convolution launchers: the
caller's filter cache (mpsr_net_opts.filter_cache / _valid / _tags) and the filter transform that rides on the
preceding 1x1 layer's launch.  Whatever the route -- no cache, a cache being filled, a valid one, one too short for
its last layer, one without tags, another cache or another entry point in between, a refused call in between -- the
trunk computes the same bits.

Geometry: the half-width trunk of tests/test_net_shapes_gpu.py on (B, H, W) = (3, 21, 23).  Block2's 3x3 layers run the
sixteen-product F(3x3,3x3) kernel on 6x6 maps there, each behind a 1x1 layer; block3's stay on the implicit GEMM.  The
entry points are called directly (DeviceNet.trunk always passes a cache).  Every call runs on a workspace filled with
0xFF bytes and writes into an output that held NaN; every new cache holds NaN.
"""
import ctypes

import pytest
import torch

import net_shape_cases as C

pytestmark = pytest.mark.gpu

B, H, WD = 3, 21, 23
MPSR_ERR_WORKSPACE = 3


class Cache:
    """A caller's filter cache of `floats` floats (NaN), with zeroed tags or none."""

    def __init__(self, part, floats, tags=True):
        self.buf = torch.full((int(floats),), float("nan"), device="cuda")
        self.tags = (ctypes.c_int32 * part.n)() if tags else None

    def opts(self, valid):
        from monopsr_amd import _lib
        o = _lib.NetOpts()
        o.filter_cache, o.filter_cache_floats, o.filter_cache_valid = self.buf.data_ptr(), self.buf.numel(), valid
        if self.tags is not None:
            o.filter_cache_tags = self.tags
        return o


def _fbytes(n):
    return (4 * n + 255) // 256 * 256


class Trunk:
    def __init__(self):
        from monopsr_amd import _lib
        from monopsr_amd.core import device_net as dn
        from monopsr_amd.core import weights as W
        self.lib = _lib.lib()
        weights = W.synthetic_weights(seed=41, width_div=2, decoder=False, heads=False)
        self.part = dn.PackedPart(*W.pack_trunk(weights, W.CROP_SCOPE, 2), torch.device("cuda"))
        g = torch.Generator(device="cuda").manual_seed(H * 1000 + WD)
        self.img = torch.randn((B, H, WD, 3), device="cuda", generator=g) * 50
        self.ws_bytes = self.lib.mpsr_trunk_workspace_bytes(B, H, WD)
        self.cache_floats = self.lib.mpsr_filter_cache_floats(self.part.layers, self.part.n)

    def records_bytes(self):
        """The workspace THESE layer records need.  mpsr_trunk_workspace_bytes sizes the full-width network (1024- and
        256-channel tensors); mpsr_trunk_fwd carves cols, root, pooled, 3 tensors of the widest layer, 2 of the widest
        3x3 layer and the launches' scratch (the same for both widths), each rounded up to 256 bytes."""
        recs = self.part.records
        oh, ow = (H - 1) // 2 + 1, (WD - 1) // 2 + 1
        ph, pw = C.trunk_map(H, WD)
        mr, mp = B * oh * ow, B * ph * pw
        scratch = self.ws_bytes - (_fbytes(mr * 160) + _fbytes(mr * 64) + _fbytes(mp * 64) + 3 * _fbytes(mp * 1024) +
                                   2 * _fbytes(mp * 256))
        cmax = max(r["cout"] for r in recs[1:])
        bmax = max(r["cout"] for r in recs[1:] if r["kh"] == 3)
        return (_fbytes(mr * recs[0]["cin"]) + _fbytes(mr * recs[0]["cout"]) + _fbytes(mp * recs[0]["cout"]) +
                3 * _fbytes(mp * cmax) + 2 * _fbytes(mp * bmax) + scratch)

    def run(self, opts=None, ex=True, ws_bytes=None):
        """-> (status, out).  ex=False: mpsr_trunk_fwd, which takes no opts."""
        from monopsr_amd import _lib
        part, lib = self.part, self.lib
        ph, pw = C.trunk_map(H, WD)
        out = torch.full((B, ph, pw, part.records[-1]["cout"]), float("nan"), device="cuda")
        ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device="cuda").fill_(0xFF)
        n = self.ws_bytes if ws_bytes is None else ws_bytes
        head = (_lib.ptr(self.img), B, H, WD, _lib.ptr(part.blob), part.layers, part.n, _lib.ptr(out), _lib.ptr(ws), n)
        if ex:
            st = lib.mpsr_trunk_fwd_ex(*head, ctypes.byref(opts) if opts is not None else None, _lib.stream())
        else:
            st = lib.mpsr_trunk_fwd(*head, _lib.stream())
        torch.cuda.synchronize()
        return st, out

    def good(self, opts=None, **kw):
        from monopsr_amd import _lib
        st, out = self.run(opts, **kw)
        _lib.check(st)
        return out


class Decoder:
    """The half-width decoder at the smallest geometry of the sweep whose plan holds a tap GEMM: its GEMMs are launches of
    the pointwise kernel that no network entry point's 1x1 layer made."""

    def __init__(self):
        from monopsr_amd import _lib
        from monopsr_amd.core import device_net as dn
        from monopsr_amd.core import weights as W
        self.lib = _lib.lib()
        tap = [c for c in C.DECODER_CASES if 7 in c.kinds]
        self.case = case = min(tap, key=lambda c: c.B * c.mh * c.mw)
        assert 7 in C.decoder_plan(case, 2)[0], "%s: no tap GEMM in the plan" % case.name
        weights = W.synthetic_weights(seed=23, width_div=2, trunk=False, heads=False)
        self.part = dn.PackedPart(*W.pack_decoder(weights, 2), torch.device("cuda"))
        g = torch.Generator(device="cuda").manual_seed(77)
        shape = (case.B, case.fh, case.fw, 512)
        self.crop = torch.randn(shape, device="cuda", generator=g).clamp_(min=0)
        self.full = torch.randn(shape, device="cuda", generator=g).clamp_(min=0)

    def run(self):
        from monopsr_amd import _lib
        case, part, lib = self.case, self.part, self.lib
        recs = part.records
        nan = lambda *s: torch.full(s, float("nan"), device="cuda")
        box = nan(case.B, case.fh // 2, case.fw // 2, recs[1]["cout"])
        fmap = nan(case.B, case.mh, case.mw, recs[5]["cout"])
        xyz = nan(case.B, case.mh, case.mw, recs[6]["cout"])
        nbytes = lib.mpsr_decoder_workspace_bytes(case.B, case.fh, case.fw, case.mh, case.mw)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda").fill_(0xFF)
        opts = Cache(part, lib.mpsr_filter_cache_floats(part.layers, part.n)).opts(0)
        _lib.check(lib.mpsr_squash_decoder_fwd_ex(_lib.ptr(self.crop), _lib.ptr(self.full), case.B, case.fh, case.fw,
                                                  case.mh, case.mw, _lib.ptr(part.blob), part.layers, part.n,
                                                  _lib.ptr(box), _lib.ptr(fmap), _lib.ptr(xyz), _lib.ptr(ws), nbytes,
                                                  ctypes.byref(opts), _lib.stream()))
        torch.cuda.synchronize()
        return box, fmap, xyz


@pytest.fixture(scope="module")
def ctx():
    """The decoder's result from before any trunk call of this module, then the trunk's without any opts."""
    dec = Decoder()
    dec_before = dec.run()
    trunk = Trunk()
    assert C.trunk_plan(B, H, WD) == (4, 0)
    first = trunk.good(ex=False)
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    return trunk, first, dec, dec_before


def _every_route(trunk, first):
    n, part = trunk.cache_floats, trunk.part
    assert n > 0
    assert torch.equal(trunk.good(None), first), "mpsr_trunk_fwd_ex without opts"
    # a cache being filled, then trusted: same bits, and the trusted call leaves the tags as the filling call wrote them
    full = Cache(part, n)
    assert torch.equal(trunk.good(full.opts(0)), first), "full cache, valid = 0"
    tags_filled = list(full.tags)
    assert any(tags_filled), "no layer noted what its slice holds"
    assert torch.equal(trunk.good(full.opts(1)), first), "full cache, valid = 1"
    assert list(full.tags) == tags_filled
    # one float short: the last 3x3 layer gets no slice and transforms into scratch both times
    short = Cache(part, n - 1)
    for valid in (0, 1):
        assert torch.equal(trunk.good(short.opts(valid)), first), "cache one float short, valid = %d" % valid
    # no tags: `valid` alone says what the slices hold
    untagged = Cache(part, n, tags=False)
    for valid in (0, 1):
        assert torch.equal(trunk.good(untagged.opts(valid)), first), "cache without tags, valid = %d" % valid
    # the first cache again: the calls that used the others left its slices and tags alone
    assert torch.equal(trunk.good(full.opts(1)), first), "full cache again, valid = 1"
    assert list(full.tags) == tags_filled


def test_every_route_of_the_filters_gives_the_same_bits(ctx):
    trunk, first, _, _ = ctx
    _every_route(trunk, first)


def test_every_route_with_the_transform_on_the_1x1_launch(ctx):
    """The same with the persistent pointwise kernel forced onto every 1x1 layer it takes (by itself it wants 512 tiles,
    ~49000 rows): block2's 1x1 layers then carry the transform of the 3x3 layer behind them, into the cache slice or into
    scratch.  Other kernels, other bits: the reference is the call without opts under the same setting."""
    trunk = ctx[0]
    trunk.lib.mpsr_debug_set_conv_pointwise(1)
    try:
        first = trunk.good(ex=False)
        assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
        _every_route(trunk, first)
    finally:
        trunk.lib.mpsr_debug_set_conv_pointwise(-1)


def test_a_decoder_call_in_between_changes_neither_result(ctx):
    trunk, first, dec, dec_before = ctx
    trunk.good(Cache(trunk.part, trunk.cache_floats).opts(0))
    again = dec.run()
    fresh = Cache(trunk.part, trunk.cache_floats)
    assert torch.equal(trunk.good(fresh.opts(0)), first), "trunk after a decoder call, cache not yet valid"
    assert torch.equal(trunk.good(fresh.opts(1)), first), "... and on the cache that call filled"
    for name, a, b in zip(("features_for_box_3d", "features_for_map", "inst_xyz_map_local"), again, dec_before):
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a, b), "decoder %s differs from before the trunk calls" % name


def test_a_refused_call_in_between_leaves_nothing_behind(ctx):
    """A workspace 256 bytes short of what the layer records need: refused by the host-side carve-up, before any launch."""
    trunk, first, _, _ = ctx
    need = trunk.records_bytes()
    assert need <= trunk.ws_bytes
    cache = Cache(trunk.part, trunk.cache_floats)
    st, out = trunk.run(cache.opts(0), ws_bytes=need - 256)
    assert st == MPSR_ERR_WORKSPACE, "status %d: %s" % (st, trunk.lib.mpsr_last_error().decode())
    assert bool(torch.isnan(out).all()) and not any(cache.tags)
    assert torch.equal(trunk.good(cache.opts(0), ws_bytes=need), first), "next call, on exactly the bytes needed"
    assert torch.equal(trunk.good(None), first)
    assert torch.equal(trunk.good(ex=False), first)
