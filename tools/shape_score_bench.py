"""Device time of mpsr_shape_scores next to what one would compose without it, with HIP events, on synthetic clouds of
2304 points (48 x 48) per box: 32 boxes with a ~25 % mask, 32 boxes with null masks, and 256 boxes with the mask.

The composition: tf_nndistance.nn_distance on the same clouds, the points that are not valid moved 1e6 m away first
(nn_distance takes no mask), then the torch reductions that give the same table -- the valid counts, the fp64 sums of
the roots and of the squares, the maxima, the counts within each threshold, and the table's arithmetic.  It is checked
against the fused call's table before it is timed.  Each window runs for at least --seconds after a warm-up; the time
of a call is the events' span over the number of calls queued between them.  Numbers: DESIGN.md section 7.14.

--surface times mpsr_surface_scores next to mpsr_shape_scores on the same clouds instead: 32
and 256 boxes of 48 x 48, a bumpy sheet with a spacing of 8 cm (a car's) and the same sheet with 3 cm of noise, with a
~25 % mask and with null masks, at max_edge 0.5 m and +inf.  It prints the kept triangles per side next to the times.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monopsr_amd.core import distance_metrics  # noqa: E402
from monopsr_amd.tf_ops.nn_distance import tf_nndistance  # noqa: E402

POINTS = 48 * 48
FAR = 1.0e6


def window(fn, seconds, warmup=5, batch=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, total_ms = 0, 0.0
    while total_ms < 1e3 * seconds:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(batch):
            fn()
        end.record()
        end.synchronize()
        total_ms += start.elapsed_time(end)
        calls += batch
    return 1e3 * total_ms / calls  # microseconds per call


def composed(a, b, mask_a, mask_b, thresholds):
    """The table of shape_scores from nn_distance and torch reductions (a box with an empty side is not handled)."""
    far = torch.full_like(a[:1, :1], FAR)
    sa = a if mask_a is None else torch.where(mask_a[..., None] > 0, a, far)
    sb = b if mask_b is None else torch.where(mask_b[..., None] > 0, b, far)
    d1, _, d2, _ = tf_nndistance.nn_distance(sa, sb)
    limits = torch.tensor([t * t for t in thresholds], dtype=torch.float64, device=a.device)
    sides = []
    for d, mask in ((d1, mask_a), (d2, mask_b)):
        ok = torch.ones_like(d, dtype=torch.bool) if mask is None else mask > 0
        dd = torch.where(ok, d.double(), torch.zeros((), dtype=torch.float64, device=d.device))
        n = ok.sum(1).double()
        within = (ok[..., None] & (dd[..., None] <= limits)).sum(1).double()
        sides.append((n, dd.sqrt().sum(1), dd.sum(1), dd.amax(1), within))
    (na, ra, qa, xa, wa), (nb, rb, qb, xb, wb) = sides
    acc, comp = ra / na, rb / nb
    p, r = wa / na[:, None], wb / nb[:, None]
    f = torch.where(p + r == 0, torch.zeros_like(p), 2 * p * r / (p + r))
    head = torch.stack([acc, comp, (acc + comp) / 2, qa / na + qb / nb, torch.maximum(xa, xb).sqrt()], 1)
    return torch.cat([head, torch.stack([p, r, f], 2).reshape(len(acc), -1)], 1).float()


def surface(seconds, dev):
    """mpsr_surface_scores against mpsr_shape_scores on sheets of 48 x 48 points."""
    thr = distance_metrics.DEFAULT_SHAPE_THRESHOLDS
    i, j = torch.meshgrid(torch.arange(48.0, device=dev), torch.arange(48.0, device=dev), indexing='ij')
    sheet = torch.stack([0.08 * i, 0.08 * j, 0.3 * torch.sin(0.4 * i) * torch.cos(0.3 * j)], -1)
    for n in (32, 256):
        for masked in (True, False):
            g = torch.Generator(device=dev).manual_seed(n + masked)
            pa = (sheet[None] + torch.randn((n, 48, 48, 3), device=dev, generator=g) * 0.01).contiguous()
            pb = pa + torch.randn((n, 48, 48, 3), device=dev, generator=g) * 0.03
            ma = (torch.rand((n, POINTS), device=dev, generator=g) < 0.25).float() if masked else None
            mb = (torch.rand((n, POINTS), device=dev, generator=g) < 0.25).float() if masked else None
            point_us = window(lambda: distance_metrics.shape_scores(pa, pb, ma, mb, thr), seconds)
            for max_edge in (0.5, float('inf')):
                s = distance_metrics.surface_scores(pa, pb, ma, mb, thr, max_edge)
                tris = s.tri_counts.double().mean(0).cpu().tolist()
                # (with null masks a call takes milliseconds: two to a batch keep the window near its length)
                us = window(lambda: distance_metrics.surface_scores(pa, pb, ma, mb, thr, max_edge), seconds, batch=2)
                print('%3d boxes of 48 x 48, %s, max_edge %3g: mpsr_surface_scores %9.1f us (%6.0f and %6.0f triangles '
                      'a box), mpsr_shape_scores %8.1f us' % (n, 'a ~25 % mask' if masked else 'null masks  ', max_edge,
                                                             us, tris[0], tris[1], point_us))
    return 0


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--seconds', type=float, default=1.0, help='length of a timing window (default 1 s)')
    p.add_argument('--surface', action='store_true',
                   help='time mpsr_surface_scores against mpsr_shape_scores instead (DESIGN.md section 7.15)')
    a = p.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    if a.surface:
        return surface(a.seconds, dev)
    thr = distance_metrics.DEFAULT_SHAPE_THRESHOLDS
    for n, masked in ((32, True), (32, False), (256, True)):
        g = torch.Generator(device=dev).manual_seed(n + masked)
        pa = torch.randn((n, POINTS, 3), device=dev, generator=g) * 2
        pb = pa + torch.randn((n, POINTS, 3), device=dev, generator=g) * 0.1
        ma = (torch.rand((n, POINTS), device=dev, generator=g) < 0.25).float() if masked else None
        mb = (torch.rand((n, POINTS), device=dev, generator=g) < 0.25).float() if masked else None
        fused = distance_metrics.shape_scores(pa, pb, ma, mb, thr).table
        other = composed(pa, pb, ma, mb, thr)
        assert torch.allclose(fused, other, rtol=1e-5, atol=1e-7), float((fused - other).abs().max())
        fused_us = window(lambda: distance_metrics.shape_scores(pa, pb, ma, mb, thr), a.seconds)
        composed_us = window(lambda: composed(pa, pb, ma, mb, thr), a.seconds)
        print('%3d boxes of %d x %d points, %s: mpsr_shape_scores %8.1f us, nn_distance + torch reductions %8.1f us'
              % (n, POINTS, POINTS, 'a ~25 % mask' if masked else 'null masks  ', fused_us, composed_us))
    return 0


if __name__ == '__main__':
    sys.exit(main())
