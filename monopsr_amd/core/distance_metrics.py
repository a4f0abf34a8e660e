"""Shape metrics over valid points: accuracy, completeness, Chamfer-L1, Hausdorff and precision / recall / F-score at
distance thresholds.

The reference's module of this name holds only its sklearn Chamfer distance.  Its two shape numbers, METRIC_EMD and
METRIC_CHAMFER (MonoPSRModel.evaluate_predictions), multiply both clouds by the valid mask and then match all 48 x 48
points, the masked ones at the object's origin included; they are kept as they are for the reference's CSVs.  The
scores here are taken over the valid points only, in metres:

    accuracy      the mean distance of a valid point of a to its nearest valid point of b
    completeness  the same from b to a
    chamfer_l1    (accuracy + completeness) / 2
    chamfer_sq    the mean squared distance a -> b plus the mean squared distance b -> a
    hausdorff     the largest of all those nearest distances
    precision_t   the share of a's valid points within t of b;  recall_t the share of b's within t of a
    fscore_t      2 precision recall / (precision + recall), 0 when both are 0

By convention a is the prediction and b the ground truth.  shape_scores is one mpsr_shape_scores call
(include/monopsr_hip.h holds the exact definitions): a fused masked nearest-neighbour search with fp64 sums in a fixed
order, so two calls return the same bytes.  chunk_shape_scores scores a chunk of the evaluator's pass, in the object's
own frame (shape alone) or placed in the camera frame (shape and localisation).

DEFAULT_SHAPE_THRESHOLDS, 5, 10 and 20 cm, is an assumption of this package, not a convention of KITTI or of the
reference: 1 - 5 % of a car's length.  So is DEFAULT_SHAPE_MAX_EDGE, 0.5 m, the longest 3-D edge a triangle of
surface_scores may have: about six grid spacings of a car (its map points are 6 - 9 cm apart) and well under the gap
between a car and its background.

surface_scores gives the same scores with the distance of a point taken to the other map's
triangulated surface instead of to its nearest point: the points of a car are as far apart as the tight thresholds, so
the point scores partly measure how two grids interleave.  One mpsr_surface_scores call; chunk_surface_scores is
chunk_shape_scores on it.
"""
import collections
import ctypes

# metres; an assumption: 1 - 5 % of the length of a car (about 4 m)
DEFAULT_SHAPE_THRESHOLDS = (0.05, 0.1, 0.2)
MAX_THRESHOLDS = 8  # MPSR_SHAPE_MAX_THRESHOLDS
# metres; an assumption: about six grid spacings of a car, well under a car-to-background gap
DEFAULT_SHAPE_MAX_EDGE = 0.5

# counts (n, 2 + 2T) int32: n_a, n_b, within_a[t], within_b[t]; sums (n, 6) float64: sum sqrt d_a, sum d_a, sum sqrt
# d_b, sum d_b, max d_a, max d_b; table (n, 5 + 3T) float32 in the order of names; dist_a (n, P) and dist_b (n, Q)
# float32 squared distances (NaN at the points that are not valid), or None
ShapeScores = collections.namedtuple('ShapeScores', ('counts', 'sums', 'table', 'dist_a', 'dist_b', 'names'))

# ShapeScores with dist_a and dist_b (n, h w) FLOAT64 and tri_counts (n, 2) int32: the kept triangles of a and of b
SurfaceScores = collections.namedtuple('SurfaceScores', ('counts', 'sums', 'table', 'dist_a', 'dist_b', 'tri_counts',
                                                         'names'))


def shape_metric_names(thresholds=DEFAULT_SHAPE_THRESHOLDS, prefix=''):
    """The columns of mpsr_shape_scores' table: prefix + accuracy, completeness, chamfer_l1, chamfer_sq, hausdorff,
    then precision_<t>, recall_<t>, fscore_<t> per threshold, <t> as '%g'."""
    names = ['accuracy', 'completeness', 'chamfer_l1', 'chamfer_sq', 'hausdorff']
    for t in thresholds:
        names += ['precision_%g' % t, 'recall_%g' % t, 'fscore_%g' % t]
    return tuple(prefix + n for n in names)


def check_thresholds(thresholds):
    """-> the thresholds as a tuple of floats; ValueError for what mpsr_shape_scores would refuse."""
    t = tuple(float(v) for v in thresholds)
    if len(t) > MAX_THRESHOLDS:
        raise ValueError('%d thresholds, more than %d' % (len(t), MAX_THRESHOLDS))
    for k, v in enumerate(t):
        if not (v > 0.0 and v != float('inf')):
            raise ValueError('thresholds[%d] = %r is not a finite distance > 0' % (k, v))
        if k and not v > t[k - 1]:
            raise ValueError('thresholds[%d] = %r is not increasing (after %r)' % (k, v, t[k - 1]))
    return t


def check_max_edge(max_edge):
    """-> max_edge as a float; ValueError for what mpsr_surface_scores would refuse (NaN, negative)."""
    v = float(max_edge)
    if not v >= 0.0:
        raise ValueError('max_edge = %r is not a length >= 0' % (max_edge,))
    return v


def _mask(who, clouds, name, t, n, points, device):
    """Mask `name` of `who` (`clouds`: its word for the inputs) as (n, points) on `device`, or None."""
    import torch
    from monopsr_amd import _lib
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() < 1 or \
            t.numel() != n * points or int(t.shape[0]) != n:
        raise _lib.InvalidArgumentError('%s: %s must hold one float32 entry per point (%d x %d)' % (
            who, name, n, points))
    if not t.is_cuda or t.device != device:
        raise _lib.InvalidArgumentError('%s: %s is not on the %s\' GPU' % (who, name, clouds))
    return t.reshape(n, points).contiguous()


def _outputs(n, T, workspace_bytes, dev):
    """-> counts, sums, table and a workspace of workspace_bytes (the current device is dev's)"""
    import torch
    return (torch.empty((n, 2 + 2 * T), dtype=torch.int32, device=dev),
            torch.empty((n, 6), dtype=torch.float64, device=dev),
            torch.empty((n, 5 + 3 * T), dtype=torch.float32, device=dev),
            torch.empty(((workspace_bytes + 7) // 8,), dtype=torch.float64, device=dev))


def shape_scores(points_a, points_b, mask_a=None, mask_b=None, thresholds=DEFAULT_SHAPE_THRESHOLDS, want_dists=False):
    """One mpsr_shape_scores call.  points_a (n, P, 3) or (n, h, w, 3) and points_b (n, Q, 3) or (n, h, w, 3) float32
    CUDA tensors; mask_a and mask_b float32 with one entry per point, or None (every point with finite coordinates is
    valid).  A point is valid when its mask entry is > 0 and its coordinates are finite.  thresholds: at most
    MAX_THRESHOLDS increasing distances in metres.  -> ShapeScores of device tensors; dist_a and dist_b are None
    without want_dists."""
    import torch
    from monopsr_amd import _lib

    def cloud(name, t):
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or int(t.shape[-1]) != 3 or \
                t.dtype != torch.float32:
            raise _lib.InvalidArgumentError('shape_scores: %s must be (n, P, 3) or (n, h, w, 3) float32, got %s' % (
                name, (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t)))
        points = int(t.shape[1]) if t.dim() == 3 else int(t.shape[1]) * int(t.shape[2])
        return t.reshape(int(t.shape[0]), points, 3)

    a, b = cloud('points_a', points_a), cloud('points_b', points_b)
    for name, t in (('points_a', a), ('points_b', b)):
        if not t.is_cuda:
            raise _lib.InvalidArgumentError('shape_scores: %s is not on the GPU; there is no CPU path' % name)
    a, b = a.contiguous(), b.contiguous()
    n, P, Q = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if int(b.shape[0]) != n or b.device != a.device:
        raise _lib.InvalidArgumentError('shape_scores: %d boxes in points_a, %d in points_b (or two devices)' % (
            n, int(b.shape[0])))

    ma = _mask('shape_scores', 'clouds', 'mask_a', mask_a, n, P, a.device)
    mb = _mask('shape_scores', 'clouds', 'mask_b', mask_b, n, Q, a.device)
    try:
        thr = check_thresholds(thresholds)
    except ValueError as e:
        raise _lib.InvalidArgumentError('shape_scores: %s' % e)
    T, dev = len(thr), a.device
    with torch.cuda.device(dev):
        lib = _lib.lib()
        counts, sums, table, workspace = _outputs(n, T, int(lib.mpsr_shape_scores_workspace_bytes(n, P, Q, T)), dev)
        dist_a = torch.empty((n, P), dtype=torch.float32, device=dev) if want_dists else None
        dist_b = torch.empty((n, Q), dtype=torch.float32, device=dev) if want_dists else None
        p = _lib.ptr
        _lib.check(lib.mpsr_shape_scores(
            p(a), p(ma), P, p(b), p(mb), Q, n, (ctypes.c_double * max(T, 1))(*thr), T, p(workspace),
            workspace.numel() * 8, p(counts), p(sums), p(table), p(dist_a), p(dist_b), _lib.stream()))
    return ShapeScores(counts, sums, table, dist_a, dist_b, shape_metric_names(thr))


def surface_scores(points_a, points_b, mask_a=None, mask_b=None, thresholds=DEFAULT_SHAPE_THRESHOLDS,
                   max_edge=DEFAULT_SHAPE_MAX_EDGE, want_dists=False):
    """One mpsr_surface_scores call.  points_a and points_b (n, h, w, 3) float32 CUDA tensors of one grid size; mask_a
    and mask_b float32 with one entry per point, or None; validity and thresholds as shape_scores takes them.  max_edge:
    the longest 3-D edge of a kept triangle in metres, >= 0, inf allowed.  -> SurfaceScores of device tensors; dist_a
    and dist_b (float64) are None without want_dists."""
    import torch
    from monopsr_amd import _lib

    for name, t in (('points_a', points_a), ('points_b', points_b)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or int(t.shape[-1]) != 3 or t.dtype != torch.float32:
            raise _lib.InvalidArgumentError('surface_scores: %s must be (n, h, w, 3) float32, got %s' % (
                name, (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t)))
        if not t.is_cuda:
            raise _lib.InvalidArgumentError('surface_scores: %s is not on the GPU; there is no CPU path' % name)
    n, h, w = (int(v) for v in points_a.shape[:3])
    if tuple(points_b.shape) != tuple(points_a.shape) or points_b.device != points_a.device:
        raise _lib.InvalidArgumentError('surface_scores: points_a is %s, points_b %s (or two devices)' % (
            tuple(points_a.shape), tuple(points_b.shape)))
    if h < 1 or w < 1:
        raise _lib.InvalidArgumentError('surface_scores: a grid of %d x %d has no point' % (h, w))
    a, b = points_a.contiguous(), points_b.contiguous()

    ma = _mask('surface_scores', 'grids', 'mask_a', mask_a, n, h * w, a.device)
    mb = _mask('surface_scores', 'grids', 'mask_b', mask_b, n, h * w, a.device)
    try:
        thr, edge = check_thresholds(thresholds), check_max_edge(max_edge)
    except ValueError as e:
        raise _lib.InvalidArgumentError('surface_scores: %s' % e)
    T, dev = len(thr), a.device
    with torch.cuda.device(dev):
        lib = _lib.lib()
        counts, sums, table, workspace = _outputs(n, T, int(lib.mpsr_surface_scores_workspace_bytes(n, h, w, T)), dev)
        tri_counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
        dist_a = torch.empty((n, h * w), dtype=torch.float64, device=dev) if want_dists else None
        dist_b = torch.empty((n, h * w), dtype=torch.float64, device=dev) if want_dists else None
        p = _lib.ptr
        _lib.check(lib.mpsr_surface_scores(
            p(a), p(ma), p(b), p(mb), n, h, w, (ctypes.c_double * max(T, 1))(*thr), T, edge, p(workspace),
            workspace.numel() * 8, p(counts), p(sums), p(table), p(dist_a), p(dist_b), p(tri_counts), _lib.stream()))
    return SurfaceScores(counts, sums, table, dist_a, dist_b, tri_counts, shape_metric_names(thr))


def _chunk_scores(who, score, model, samples, outs, placed):
    """The body of chunk_shape_scores and chunk_surface_scores (`who`): score(a, b, mask) on the clouds of the object's
    own frame and, with placed, of the camera frame; a and b (n,) + roi + (3,)."""
    import torch
    if len(samples) != len(outs):
        raise ValueError('%d samples, %d outputs' % (len(samples), len(outs)))
    if len(samples) == 0:
        raise ValueError('%s needs at least one frame' % who)
    with torch.cuda.device(samples[0]['gt_valid_mask_maps'].device), torch.no_grad():
        roi, local, gt_local, mask, glob, gt_global = _chunk_clouds(model, samples, outs, placed)
        grid = lambda t: t.reshape((int(t.shape[0]),) + roi + (3,))
        shape = score(grid(local), grid(gt_local), mask)
        return shape, score(grid(glob), grid(gt_global), mask) if placed else None


def _chunk_clouds(model, samples, outs, placed):
    """The clouds and the mask chunk_shape_scores and chunk_surface_scores score: -> (roi, local, gt_local, mask,
    placed cloud or None, gt_global or None)."""
    import torch
    from monopsr_amd.core import constants
    from monopsr_amd.datasets.kitti import instance_utils
    roi = tuple(model.map_roi_size)
    counts = [int(s['num_objs']) for s in samples]
    cat = lambda ts, tail: torch.cat([t[0:n].reshape((n,) + tail).float() for t, n in zip(ts, counts)], 0)
    local = cat([o[constants.KEY_INST_XYZ_MAP_LOCAL] for o in outs], roi + (3,))
    mask = cat([s['gt_valid_mask_maps'] for s in samples], roi)
    gt_local = cat([s['gt_inst_xyz_maps_local'] for s in samples], roi + (3,))
    if not placed:
        return roi, local, gt_local, mask, None, None
    view = cat([o[constants.KEY_VIEW_ANG] for o in outs], (1,))
    cen = cat([o[constants.KEY_CENTROIDS] for o in outs], (3,))
    glob = instance_utils.tf_inst_xyz_map_local_to_global(local, roi, view, cen)
    gt_global = cat([s['gt_inst_xyz_maps_global'] for s in samples], roi + (3,))
    return roi, local, gt_local, mask, glob, gt_global


def chunk_surface_scores(model, samples, outs, thresholds=DEFAULT_SHAPE_THRESHOLDS, max_edge=DEFAULT_SHAPE_MAX_EDGE,
                         placed=False):
    """chunk_shape_scores against surfaces: exactly its clouds and masks (the same tensor operations on the same
    inputs), each scored by surface_scores with max_edge.  -> (SurfaceScores, SurfaceScores or None)."""
    return _chunk_scores('chunk_surface_scores', lambda a, b, m: surface_scores(a, b, m, m, thresholds, max_edge),
                         model, samples, outs, placed)


def chunk_shape_scores(model, samples, outs, thresholds=DEFAULT_SHAPE_THRESHOLDS, placed=False):
    """The shape scores of a chunk of the evaluator's pass: `samples` as dataset.get_sample_dict returns them ('val'
    mode), `outs` as model.build_batch returns them.  The first num_objs rows of every frame, frame after frame, as
    scene_reconstruction.reconstruct_frames concatenates them; one launch (two with placed).
    In the object's frame: a = outs[KEY_INST_XYZ_MAP_LOCAL], b = gt_inst_xyz_maps_local, both masks the sample's
    gt_valid_mask_maps.  placed: a = instance_utils.tf_inst_xyz_map_local_to_global of the same maps with KEY_VIEW_ANG
    and KEY_CENTROIDS, the cloud reconstruct_frames places (so the fitted one after instance_metrics.fit_centroids),
    b = gt_inst_xyz_maps_global.  -> (ShapeScores, ShapeScores or None)."""
    return _chunk_scores('chunk_shape_scores', lambda a, b, m: shape_scores(a, b, m, m, thresholds), model, samples,
                         outs, placed)
