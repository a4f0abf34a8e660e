"""Shapes of the transform-domain weight-gradient sweep (tests/test_wgrad_shapes.py on the host, tests/test_wgrad_shapes_gpu.py
on the device), the schedule each is meant to reach and the helpers both files share.

Both kernels (csrc/winograd4_wgrad.hip: F(4x4,3x3), K step = 8 tiles; csrc/winograd3_wgrad.hip: F(3x3,3x3), K step = 4
tiles) cut the tile sum into slices of an even number of K steps, zero-fill the tiles past the last one through
out-of-range buffer offsets, decode tiles with FastDiv and meet in dw through fp32 atomics -- and both have a size floor
(B * H * W >= 131072 pixels; B * dilation^2 >= 2048 tiles) that no small random sweep passes.  Every shape below is the
smallest that passes the floor and still reaches the edge its comment names.  The schedule columns restate the launchers'
arithmetic (restated_schedule below); mpsr_conv2d_wgrad_plan -- the launchers' own helper -- is asserted against them per
case, so a retuned threshold or slice rule shows up as a failed plan assertion instead of a sweep that quietly stopped
reaching its edge.
"""
import ctypes

KT = {3: 8, 4: 4}            # tiles per K step of kind 3 (F(4x4,3x3)) and kind 4 (F(3x3,3x3))
WORKGROUPS = {3: 512, 4: 256}  # workgroups a launch aims at
BLOCK = {3: 32, 4: 64}       # side of a workgroup's (n, c) block
FLOOR_PIXELS = 131072        # winograd4_wgrad_applies: B * H * W
FLOOR_TILES = 2048           # winograd3_wgrad_applies: B * dilation^2


class WgradCase:
    def __init__(self, name, kind, B, H, W, C, N, dil, tiles, steps_raw, steps, nslices, last_live, edges, what):
        self.name, self.kind = name, kind
        self.B, self.H, self.W, self.C, self.N, self.dil = B, H, W, C, N, dil
        # the schedule: tiles, K steps per slice before and after rounding to even, slices, live tiles of the last slice
        self.tiles, self.steps_raw, self.steps, self.nslices, self.last_live = tiles, steps_raw, steps, nslices, last_live
        self.edges = edges  # predicate name (EDGE_PREDICATES) -> the value the case exists for
        self.what = what

    def __repr__(self):
        return self.name

    @property
    def shape(self):
        return (self.B, self.H, self.W, self.C, self.N)

    @property
    def pixels(self):
        return self.B * self.H * self.W

    @property
    def tiles_per_image(self):
        return (self.H // 4) * (self.W // 4) if self.kind == 3 else self.dil * self.dil

    @property
    def scratch_floats(self):
        return 36 * self.N * self.C if self.kind == 3 else 0

    @property
    def slice_capacity(self):
        return self.steps * KT[self.kind]


def _w4(name, shape, tiles, steps_raw, steps, nslices, last_live, edges, what):
    B, H, W, C, N = shape
    return WgradCase(name, 3, B, H, W, C, N, 1, tiles, steps_raw, steps, nslices, last_live, edges, what)


def _w3(name, shape, tiles, steps_raw, steps, nslices, last_live, edges, what):
    B, dil, C, N = shape
    return WgradCase(name, 4, B, 3 * dil, 3 * dil, C, N, dil, tiles, steps_raw, steps, nslices, last_live, edges, what)


# What a case can be named for, each a function of the case and of the schedule (tiles, steps, nslices) the PLAN gave.
EDGE_PREDICATES = {
    "tiles_mod_kt": lambda c, t, s, n: t % KT[c.kind],                 # != 0: the last live K step is partial
    "nslices_mod_8": lambda c, t, s, n: n % 8,                          # != 0: workgroups take the early return
    "rounded": lambda c, t, s, n: c.steps_raw != s,                     # an odd step count became even
    "last_live": lambda c, t, s, n: t - (n - 1) * s * KT[c.kind],       # live tiles of the last slice
    "dead_steps": lambda c, t, s, n: s - -(-(t - (n - 1) * s * KT[c.kind]) // KT[c.kind]),  # whole dead steps in it
    "straddle": lambda c, t, s, n: c.tiles_per_image % KT[c.kind] != 0,  # a K step holds tiles of two images
    "n_ne_c": lambda c, t, s, n: (c.N > c.C) - (c.N < c.C),             # sign of N - C
    "h_ne_w": lambda c, t, s, n: (c.H > c.W) - (c.H < c.W),             # sign of H - W
    "blocks": lambda c, t, s, n: (c.N // BLOCK[c.kind]) * (c.C // BLOCK[c.kind]),
    "tiles_high": lambda c, t, s, n: c.H // 4 if c.kind == 3 else 1,    # th: 1 = the row ring is always out of the image
    "tiles_wide": lambda c, t, s, n: c.W // 4 if c.kind == 3 else 1,    # tw: 1 = the column ring is
    "fastdiv": lambda c, t, s, n: (c.tiles_per_image, c.W // 4 if c.kind == 3 else c.dil),  # the two divisors
    "images": lambda c, t, s, n: c.B,
}


# F(4x4,3x3): (B, H, W, C, N), T, steps before -> after rounding, slices, live tiles of the last slice
W4_CASES = [
    _w4("A", (63, 44, 52, 128, 160), 9009, 36, 36, 32, 81,
        dict(tiles_mod_kt=1, straddle=True, h_ne_w=-1, tiles_wide=13, n_ne_c=1, blocks=20, dead_steps=25, rounded=False,
             nslices_mod_8=0),
        "T % 8 = 1: the last live step is partial; 143 tiles per image: steps straddle images; H != W with tw = 13, "
        "N != C with 5 x 4 blocks; the last slice has whole dead steps after a partial one"),
    _w4("B", (63, 44, 52, 192, 128), 9009, 47, 48, 24, 177,
        dict(n_ne_c=-1, blocks=24, rounded=True, tiles_mod_kt=1),
        "C > N; 24 blocks, so 24 slices; odd -> even step rounding"),
    _w4("C", (8193, 4, 4, 160, 128), 8193, 33, 34, 31, 33,
        dict(fastdiv=(1, 1), tiles_high=1, tiles_wide=1, nslices_mod_8=7, rounded=True, tiles_mod_kt=1),
        "one tile per image: FastDiv(1) twice and all four rings out of the image in every patch; nslices % 8 = 7: one "
        "group of workgroups takes the early return"),
    _w4("D1", (2049, 4, 16, 128, 160), 8196, 33, 34, 31, 36,
        dict(tiles_high=1, tiles_wide=4, h_ne_w=-1, tiles_mod_kt=4, nslices_mod_8=7),
        "th = 1 alone: only the row ring is always out of the image (transposed pair with D2: an H/W mix-up fails one)"),
    _w4("D2", (2049, 16, 4, 160, 128), 8196, 33, 34, 31, 36,
        dict(tiles_high=4, tiles_wide=1, h_ne_w=1, tiles_mod_kt=4, nslices_mod_8=7),
        "tw = 1 alone: only the column ring is always out of the image"),
    _w4("E", (29, 68, 68, 256, 288), 8381, 131, 132, 8, 989,
        dict(blocks=72, tiles_mod_kt=5, tiles_wide=17, straddle=True, rounded=True, nslices_mod_8=0),
        "72 blocks: the 8-slice minimum applies; long slices, 17 x 17 tiles, T % 8 = 5"),
    _w4("F", (1, 364, 364, 128, 128), 8281, 33, 34, 31, 121,
        dict(images=1, tiles_wide=91, fastdiv=(8281, 91), tiles_mod_kt=1, nslices_mod_8=7),
        "a single image: the first and last patch rows sit at the two ends of the buffer; tw = 91"),
    # the shape tests/test_backward_gpu.py::test_wgrad_winograd_domain_vs_direct_and_fp64 runs: everything divides
    _w4("decoder", (64, 48, 48, 128, 128), 9216, 36, 36, 32, 288,
        dict(tiles_mod_kt=0, nslices_mod_8=0, rounded=False, dead_steps=0, straddle=False, n_ne_c=0, h_ne_w=0),
        "the decoder layer: every slice full, no partial step, no rounding, no early return"),
]

# F(3x3,3x3): (B, dilation, C, N) with H = W = 3 * dilation
W3_CASES = [
    _w3("G", (2051, 1, 128, 192), 2051, 11, 12, 43, 35,
        dict(tiles_mod_kt=3, fastdiv=(1, 1), rounded=True, nslices_mod_8=3, n_ne_c=1),
        "T % 4 = 3 and FastDiv(1)"),
    _w3("H", (229, 3, 192, 128), 2061, 11, 12, 43, 45,
        dict(tiles_mod_kt=1, fastdiv=(9, 3), n_ne_c=-1, straddle=True),
        "T % 4 = 1, FastDiv of 9 and 3, C > N"),
    _w3("I", (2051, 1, 256, 256), 2051, 33, 34, 16, 11,
        dict(tiles_mod_kt=3, dead_steps=31, blocks=16, rounded=True),
        "a last slice that is almost entirely dead"),
    # the shapes tests/test_backward_gpu.py::test_wgrad_winograd3_domain_vs_direct_and_fp64 runs: T % 4 = 0 in all
    _w3("b3-128", (128, 4, 128, 192), 2048, 11, 12, 43, 32, dict(tiles_mod_kt=0, fastdiv=(16, 4)),
        "block3's conv2 at 128 crops, exactly at the floor"),
    _w3("b3-136", (136, 4, 256, 256), 2176, 34, 34, 16, 136, dict(tiles_mod_kt=0, dead_steps=0, nslices_mod_8=0),
        "full width: 16 blocks, 16 full slices"),
    _w3("b2-600", (600, 2, 128, 128), 2400, 10, 10, 60, 40, dict(tiles_mod_kt=0, fastdiv=(4, 2), dead_steps=0),
        "dilation 2"),
]

CASES = W4_CASES + W3_CASES
NEW_CASES = [c for c in CASES if len(c.name) <= 2]  # A .. I: the ragged schedules (the rest are the older tests' shapes)
BY_NAME = {c.name: c for c in CASES}


def restated_schedule(kind, tiles, C, N):
    """The launchers' slice arithmetic once more, for the table's columns: -> (steps before rounding, steps, nslices)."""
    kt, blocks = KT[kind], (N // BLOCK[kind]) * (C // BLOCK[kind])
    slices = max(8, (WORKGROUPS[kind] // blocks + 7) // 8 * 8)
    raw = -(-tiles // (slices * kt))
    steps = (raw + 1) // 2 * 2
    return raw, steps, -(-tiles // (steps * kt))


def wgrad_plan(B, H, W, C, N, k, dil, ws_floats):
    """mpsr_conv2d_wgrad_plan -> (kind, tiles, steps, nslices); host code, no GPU."""
    from monopsr_amd import _lib
    out = [ctypes.c_int(-1) for _ in range(4)]
    _lib.check(_lib.lib().mpsr_conv2d_wgrad_plan(B, H, W, C, N, k, k, dil, ws_floats, *[ctypes.byref(o) for o in out]))
    return tuple(o.value for o in out)


def case_plan(c, B=None, ws_floats=None):
    return wgrad_plan(c.B if B is None else B, c.H, c.W, c.C, c.N, 3, c.dil,
                      c.scratch_floats if ws_floats is None else ws_floats)


def check_case_plan(c):
    """Asserts the kind and the schedule the case was designed for."""
    got = case_plan(c)
    assert got == (c.kind, c.tiles, c.steps, c.nslices), "%s %s: planned %s, designed for %s" % (
        c.name, c.shape, got, (c.kind, c.tiles, c.steps, c.nslices))
    return got
