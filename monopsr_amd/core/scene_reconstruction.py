"""The output side of the reconstruction: the predicted instance clouds of a chunk of frames in the camera frame,
coloured from the image, and the same clouds rendered back into the image as a depth map and an instance image
(csrc/scene.hip).

    scene = reconstruct_frames(model, samples, outs, min_score=0.1)     # samples / outs of one Evaluator chunk
    for f, s in enumerate(samples):
        save_frame(scene_output_dirs(base), s['sample_name'], scene.frame(f))

writes <name>.ply (binary little-endian: float x y z, uchar red green blue, int box), the depth map as
depth_map_utils.save_depth_map writes a LiDAR one and the instance image as instance_utils.save_instance_image writes a
ground-truth one (255 background, k the k-th box of the frame).

The rendering is a z-buffer: the nearest point of a pixel wins, on equal float32 depth the lower point index.  (The
LiDAR projection of depth_map_utils keeps the last duplicate of a pixel, as the reference does with a LiDAR cloud.)
Colours are the image's value at the point's pixel (nearest pixel, exact).  Everything stays on the device; one copy of
n_frames + 1 offsets to the host per call tells where each frame's points are.

With ground truth (the LiDAR depth maps, the instance images and each box's instance id: what
KittiDataset.frame_ground_truth returns) the same call also scores the reconstruction per box (mpsr_scene_score, DESIGN.md
section 7.8): SceneResult.scores, a SceneScores of six exact counts and three fp64 sums per box, and its table() of
SCENE_METRIC_NAMES.  One limit: a box has 48 x 48 points, so a box larger than 48 x 48 pixels cannot fill its mask, and
scene_mask_iou is bounded by pred_px / gt_px for near objects.  That is why the two precisions and the raw counts are
reported next to it.

render_instance_surfaces lifts that limit: it joins the cells of a box's map into triangles and
rasterises them through a z-buffer of its own, so that the depth map and the instance image are dense, and scores them
the same way (SurfaceResult, SurfaceScores, SURFACE_METRIC_NAMES).  reconstruct_frames(..., surfaces={...}) renders both.
"""
import ctypes
import os

import numpy as np

from monopsr_amd import _lib

MAX_BOXES = 255  # per frame: 255 of an instance image is the background

# the columns of SceneScores.counts and .sums (mpsr_scene_score) and of SceneScores.table()
SCENE_COUNT_NAMES = ('kept', 'on_points', 'pred_px', 'inter_px', 'gt_px', 'depth_n')
SCENE_SUM_NAMES = ('sum_e', 'sum_abs_e', 'sum_e2')
SCENE_METRIC_NAMES = ('scene_mask_iou', 'scene_mask_precision', 'scene_point_precision', 'scene_depth_bias',
                      'scene_depth_mae', 'scene_depth_rmse')

# the same of SurfaceScores (mpsr_scene_surface_score)
SURFACE_COUNT_NAMES = ('tris', 'pred_px', 'inter_px', 'gt_px', 'depth_n')
SURFACE_SUM_NAMES = ('sum_e', 'sum_abs_e', 'sum_e2')
SURFACE_METRIC_NAMES = ('surface_mask_iou', 'surface_mask_precision', 'surface_mask_recall', 'surface_depth_bias',
                        'surface_depth_mae', 'surface_depth_rmse')
# the defaults of render_instance_surfaces.  1.0 m between neighbouring samples of one surface (about a quarter of a
# car's length) is an assumption, not a measurement: DESIGN.md section 7.9
SURFACE_MAX_EDGE_DZ = 1.0
SURFACE_MAX_SPAN_PX = 64

_PLY_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'),
                       ('box', '<i4')])
_PLY_HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n'
               'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int box\n'
               'end_header\n')


def _empty(shape, dtype, device):
    """Every device buffer of this module comes from here (tests/test_scene_reconstruction_gpu.py poisons them)."""
    import torch
    return torch.empty(shape, dtype=dtype, device=device)


class FrameScene(object):
    """One frame of a SceneResult: xyz (m,3), rgb (m,3) or None, box (m,) int32 = the ordinal within the frame (the
    value of the instance image), pixel (m,) int32 = row * w + col, depth_map (h,w) float32, instance_map (h,w) uint8;
    kept_per_box / visible_per_box (n,) int32 of the frame's boxes."""
    __slots__ = ('xyz', 'rgb', 'box', 'pixel', 'depth_map', 'instance_map', 'kept_per_box', 'visible_per_box')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _metric_table(count_names, third, counts, sums, box_gt_id):
    """What score_table and surface_score_table share: mask IoU, mask precision, the ratio of the two counts named by
    `third`, depth bias, MAE and RMSE from counts (B, len(count_names)), in fp64, rounded once.  A ratio whose
    denominator is 0 is NaN, and so is the IoU of a box without ground truth."""
    import torch
    col = dict(zip(count_names, counts.to(torch.float64).unbind(1)))
    pred_px, inter_px, gt_px, depth_n = (col[k] for k in ('pred_px', 'inter_px', 'gt_px', 'depth_n'))
    has_gt = (box_gt_id >= 0) & (box_gt_id <= 254)
    nan = torch.full_like(pred_px, float('nan'))
    ratio = lambda num, den, ok: torch.where(ok & (den > 0), num / torch.where(den > 0, den, torch.ones_like(den)), nan)
    every = torch.ones_like(has_gt)
    return torch.stack([ratio(inter_px, pred_px + gt_px - inter_px, has_gt), ratio(inter_px, pred_px, every),
                        ratio(col[third[0]], col[third[1]], every), ratio(sums[:, 0], depth_n, every),
                        ratio(sums[:, 1], depth_n, every), torch.sqrt(ratio(sums[:, 2], depth_n, every))],
                       1).to(torch.float32)


def score_table(counts, sums, box_gt_id):
    """The (B, 6) float32 per-box metric table in SCENE_METRIC_NAMES order from counts (B, 6) int, sums (B, 3) float64
    and box_gt_id (B,) int, tensors of one device: computed in fp64, rounded once.
        scene_mask_iou         inter_px / (pred_px + gt_px - inter_px): the IoU of the mask the box renders and the true
                               one; NaN when the box has no ground truth (id outside [0, 254]) or the union is 0
        scene_mask_precision   inter_px / pred_px; NaN when pred_px == 0
        scene_point_precision  on_points / kept; NaN when kept == 0
        scene_depth_bias       sum e / depth_n          (e = z - LiDAR depth over the depth_n points)
        scene_depth_mae        sum |e| / depth_n
        scene_depth_rmse       sqrt(sum e^2 / depth_n); all three NaN when depth_n == 0"""
    return _metric_table(SCENE_COUNT_NAMES, ('on_points', 'kept'), counts, sums, box_gt_id)


class _Scores(object):
    """counts, sums and box_gt_id of a scoring call; table(): the subclass's table function of them."""
    __slots__ = ('counts', 'sums', 'box_gt_id')

    def __init__(self, counts, sums, box_gt_id):
        self.counts, self.sums, self.box_gt_id = counts, sums, box_gt_id

    def table(self):
        return self._table(self.counts, self.sums, self.box_gt_id)


class SceneScores(_Scores):
    """A reconstruction against its ground truth, per box, device tensors: counts (B, 6) int32 (SCENE_COUNT_NAMES),
    sums (B, 3) float64 (SCENE_SUM_NAMES), box_gt_id (B,) int32 as given.  table(): score_table of them."""
    __slots__ = ()
    _table = staticmethod(score_table)


class SceneResult(object):
    """What project_instance_points returns, device tensors: xyz (M,3) float32, rgb (M,3) float32 or None, box (M,)
    int32 (index into the call's boxes), pixel (M,) int32, frame_offset (F+1,) int64 (frame f owns rows
    frame_offset[f] .. frame_offset[f+1]), depth_maps / instance_maps: lists of (H_f, W_f) float32 / uint8,
    kept_per_box / visible_per_box (B,) int32.  frame_offset_host and box_frame_host are their host copies.  scores: a
    SceneScores when the call was given ground truth, else None.  surfaces: the SurfaceResult of the same chunk when
    reconstruct_frames was asked for it, else None."""
    __slots__ = ('xyz', 'rgb', 'box', 'pixel', 'frame_offset', 'depth_maps', 'instance_maps', 'kept_per_box',
                 'visible_per_box', 'frame_offset_host', 'box_frame_host', 'scores', 'surfaces')

    def __init__(self, **kw):
        kw.setdefault('scores', None)
        kw.setdefault('surfaces', None)
        for k in self.__slots__:
            setattr(self, k, kw[k])

    @property
    def num_frames(self):
        return len(self.depth_maps)

    def frame(self, f):
        a, b = int(self.frame_offset_host[f]), int(self.frame_offset_host[f + 1])
        b0, b1 = (int(v) for v in np.searchsorted(self.box_frame_host, [f, f + 1]))
        return FrameScene(xyz=self.xyz[a:b], rgb=None if self.rgb is None else self.rgb[a:b], box=self.box[a:b] - b0,
                          pixel=self.pixel[a:b], depth_map=self.depth_maps[f], instance_map=self.instance_maps[f],
                          kept_per_box=self.kept_per_box[b0:b1], visible_per_box=self.visible_per_box[b0:b1])


def _host_ints(v):
    import torch
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v).astype(np.int32))


def _ground_truth_tables(ground_truth, hw, nb, dev):
    """-> (the F depth maps, the F instance images, box_gt_id (B,) int32 on the device), checked against the frames."""
    import torch
    nf = len(hw)
    try:
        depths, insts, ids = ground_truth['depth_maps'], ground_truth['instance_images'], ground_truth['box_gt_id']
    except (KeyError, TypeError):
        raise _lib.InvalidArgumentError("ground_truth must be a dict of 'depth_maps', 'instance_images' and 'box_gt_id'")
    if len(depths) != nf or len(insts) != nf:
        raise _lib.InvalidArgumentError('%d depth maps and %d instance images for %d frames'
                                        % (len(depths), len(insts), nf))
    out_d, out_i = [], []
    for f in range(nf):
        shape = (int(hw[f, 0]), int(hw[f, 1]))
        for what, t, dtype in (('depth map', depths[f], torch.float32), ('instance image', insts[f], torch.uint8)):
            if not torch.is_tensor(t) or not t.is_cuda or tuple(t.shape) != shape or t.dtype != dtype:
                raise _lib.InvalidArgumentError('ground truth: %s %d must be a (%d, %d) %s CUDA tensor'
                                                % (what, f, shape[0], shape[1], str(dtype).split('.')[-1]))
        out_d.append(depths[f].detach().to(dev).contiguous())  # (a view of a resident stack is taken as it is)
        out_i.append(insts[f].detach().to(dev).contiguous())
    if not torch.is_tensor(ids):
        ids = np.asarray(ids)
        ids = torch.from_numpy(np.ascontiguousarray(ids.astype(np.int64) if ids.size == 0 or ids.dtype.kind in 'iu'
                                                    else ids.astype(np.float64)))
    ids = ids.to(dev)
    if ids.dim() != 1 or ids.numel() != nb or ids.is_floating_point():
        raise _lib.InvalidArgumentError('ground truth: box_gt_id must be %d ints, got %s %s'
                                        % (nb, tuple(ids.shape), ids.dtype))
    return out_d, out_i, ids.clamp(-1, 255).to(torch.int32).contiguous()


def _frame_tables(frame_shapes, box_frame, nb):
    """-> the host tables of a chunk, checked: hw (F, 2) int32, box_frame (B,) int32, pixel offsets (F + 1,) int64."""
    nf = len(frame_shapes)
    hw = np.ascontiguousarray(np.asarray([[int(s[0]), int(s[1])] for s in frame_shapes], np.int32).reshape(nf, 2))
    if nf and int(hw.min()) <= 0:
        raise _lib.InvalidArgumentError('frame_shapes must be positive, got %s' % (hw.tolist(),))
    bf = _host_ints(box_frame).reshape(-1)
    if len(bf) != nb:
        raise _lib.InvalidArgumentError('box_frame has %d entries for %d boxes' % (len(bf), nb))
    if nb and (int(bf.min()) < 0 or int(bf.max()) >= nf or bool(np.any(np.diff(bf) < 0))):
        raise _lib.InvalidArgumentError('box_frame must lie in [0, %d) and never decrease' % nf)
    if nb and int(np.bincount(bf).max()) > MAX_BOXES:
        raise _lib.InvalidArgumentError('a frame has %d boxes, more than %d (255 of an instance image is the '
                                        'background)' % (int(np.bincount(bf).max()), MAX_BOXES))
    offs = np.zeros(nf + 1, np.int64)
    offs[1:] = np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])
    return hw, bf, offs


def _cameras(cam_p, nf, dev):
    """cam_p (a tensor, an array or a list of (3, 4)) -> (F, 3, 4) float64 on the device."""
    import torch
    if torch.is_tensor(cam_p):
        cam = cam_p.to(dev).double().reshape(-1, 3, 4).contiguous()
    else:
        cam = torch.from_numpy(np.ascontiguousarray(np.stack(
            [(c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)).astype(np.float64).reshape(3, 4)
             for c in cam_p] or [np.zeros((3, 4))]))).to(dev)
    if nf and cam.shape[0] != nf:
        raise _lib.InvalidArgumentError('%d cameras for %d frames' % (cam.shape[0], nf))
    return cam


def _mask_and_keep(valid_mask, keep, nb, npts, dev):
    """-> (valid_mask as (B, P) float32 or None, keep as (B,) int32 of 0 / 1 or None), on the device."""
    import torch
    mask = keep_d = None
    if valid_mask is not None:
        if valid_mask.numel() != nb * npts:
            raise _lib.InvalidArgumentError('valid_mask %s does not match %d boxes of %d points'
                                            % (tuple(valid_mask.shape), nb, npts))
        mask = valid_mask.detach().to(dev).to(torch.float32).reshape(nb, npts).contiguous()
    if keep is not None:
        keep_d = torch.as_tensor(keep, device=dev).reshape(-1).ne(0).to(torch.int32).contiguous()
        if keep_d.numel() != nb:
            raise _lib.InvalidArgumentError('keep has %d entries for %d boxes' % (keep_d.numel(), nb))
    return mask, keep_d


def _host(a):
    """The address of a host array, as an entry point takes it."""
    return a.ctypes.data_as(ctypes.c_void_p)


def _device_tables(hw, bf, offs, dev):
    """-> the device copies of _frame_tables' three."""
    import torch
    return torch.from_numpy(hw).to(dev), torch.from_numpy(bf).to(dev), torch.from_numpy(offs).to(dev)


def _score_args(lib, gt, nf, dev):
    """gt: what _ground_truth_tables returns -> (the device table of the depth maps' addresses, that of the instance
    images', the scratch of a scoring call), as mpsr_scene_score and mpsr_scene_surface_score take them."""
    import torch
    tables = torch.from_numpy(np.asarray([[_lib.ptr(t) for t in gt[0]], [_lib.ptr(t) for t in gt[1]]],
                                         np.uint64).view(np.int64)).to(dev)
    return tables[0], tables[1], _empty((lib.mpsr_scene_score_scratch_bytes(nf),), torch.uint8, dev)


def _fill_empty(depth, inst, scores):
    """The outputs of a chunk with nothing to launch: depth 0, instance 255, no count and no sum (gt_px is not counted
    either)."""
    depth.zero_()
    inst.fill_(255)
    if scores is not None:
        scores.counts.zero_()
        scores.sums.zero_()


def _frame_views(flat, hw, offs):
    """A flat map over all pixels of the chunk -> the list of its (h_f, w_f) views."""
    return [flat[int(offs[f]):int(offs[f + 1])].view(int(hw[f, 0]), int(hw[f, 1])) for f in range(len(hw))]


def project_instance_points(xyz_global, box_frame, cam_p, frame_shapes, images=None, valid_mask=None, keep=None,
                            visible_only=False, ground_truth=None):
    """The direct wrapper of mpsr_scene_project / _resolve / _compact (and, with ground_truth, mpsr_scene_score).

    xyz_global (B,P,3) or (B,H,W,3) float32 CUDA tensor in the camera frame; box_frame (B,) the frame of each box,
    never decreasing (a host sequence: a tensor is copied to the host); cam_p (F,3,4), a tensor, an array or a list of
    (3,4), used in float64; frame_shapes F x (h, w[, ...]); images None or F CUDA tensors (h_f, w_f, 3) float32;
    valid_mask None or (B,P) / (B,H,W[,1]) float32, a point counts where it is > 0; keep None or (B,) (bool or int): a
    box with 0 takes no part.  visible_only: the cloud holds each pixel's winner only.  ground_truth: None or a dict of
    depth_maps (F CUDA tensors (h_f, w_f) float32), instance_images (F CUDA tensors (h_f, w_f) uint8) and box_gt_id
    ((B,) ints, a tensor or a sequence: the value of each box in its frame's instance image, outside [0, 254] for a box
    without ground truth); with it the result carries .scores (SceneScores).  -> SceneResult."""
    import torch
    if not torch.is_tensor(xyz_global) or not xyz_global.is_cuda:
        raise _lib.MpsrError('expected xyz_global on the GPU; monopsr_amd has no CPU path')
    if xyz_global.dim() not in (3, 4) or xyz_global.shape[-1] != 3:
        raise _lib.InvalidArgumentError('xyz_global must be (B, P, 3) or (B, H, W, 3), got %s'
                                        % (tuple(xyz_global.shape),))
    dev = xyz_global.device
    nb = int(xyz_global.shape[0])
    npts = int(np.prod(xyz_global.shape[1:-1]))
    hw, bf, offs = _frame_tables(frame_shapes, box_frame, nb)
    nf = len(hw)
    if nb * npts >= 2 ** 32:
        raise _lib.InvalidArgumentError('%d boxes of %d points: the point index does not fit 32 bits' % (nb, npts))
    if images is not None and len(images) != nf:
        raise _lib.InvalidArgumentError('%d images for %d frames' % (len(images), nf))
    total = int(offs[-1])
    lib = _lib.lib()
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    with torch.cuda.device(dev):
        cam = _cameras(cam_p, nf, dev)
        xyz_in = xyz_global.detach().to(f32).reshape(nb, npts, 3).contiguous()
        mask, keep_d = _mask_and_keep(valid_mask, keep, nb, npts, dev)
        table = rgb = None
        imgs = []
        if images is not None:
            for f, im in enumerate(images):
                if not torch.is_tensor(im) or tuple(im.shape) != (int(hw[f, 0]), int(hw[f, 1]), 3):
                    raise _lib.InvalidArgumentError('image %d must be a (%d, %d, 3) tensor' % (f, hw[f, 0], hw[f, 1]))
                imgs.append(im.detach().to(dev).to(f32).contiguous())  # (kept alive until the launches are queued)
            table = torch.from_numpy(np.asarray([_lib.ptr(im) for im in imgs] or [0], np.uint64).view(np.int64)).to(dev)
        scores = gt = None
        if ground_truth is not None:
            gt = _ground_truth_tables(ground_truth, hw, nb, dev)
            scores = SceneScores(_empty((nb, 6), i32, dev), _empty((nb, 3), torch.float64, dev), gt[2])
        cap = nb * npts
        depth = _empty((total,), f32, dev)
        inst = _empty((total,), torch.uint8, dev)
        xyz = _empty((cap, 3), f32, dev)
        if images is not None:
            rgb = _empty((cap, 3), f32, dev)
        box, pixel = _empty((cap,), i32, dev), _empty((cap,), i32, dev)
        kept, visible = _empty((nb,), i32, dev), _empty((nb,), i32, dev)
        frame_offset = _empty((nf + 1,), i64, dev)
        if nf == 0 or cap == 0 or total == 0:  # nothing to launch: empty maps, an empty cloud
            _fill_empty(depth, inst, scores)
            kept.zero_()
            visible.zero_()
            frame_offset.zero_()
            fo_host = np.zeros(nf + 1, np.int64)
        else:
            hw_d, bf_d, offs_d = _device_tables(hw, bf, offs, dev)
            ws = _empty((lib.mpsr_scene_workspace_bytes(nf, total, nb, npts),), torch.uint8, dev)
            stream = _lib.stream()
            _lib.check(lib.mpsr_scene_project(
                _lib.ptr(xyz_in), _lib.ptr(mask), _lib.ptr(bf_d), _host(bf), _lib.ptr(keep_d), _lib.ptr(cam),
                _lib.ptr(hw_d), _host(hw), _lib.ptr(offs_d), _host(offs), nf, nb, npts, _lib.ptr(ws), ws.numel(),
                stream))
            _lib.check(lib.mpsr_scene_resolve(_lib.ptr(bf_d), _host(bf), nf, total, nb, npts, _lib.ptr(ws), ws.numel(),
                                              _lib.ptr(depth), _lib.ptr(inst), stream))
            _lib.check(lib.mpsr_scene_compact(
                _lib.ptr(xyz_in), _lib.ptr(bf_d), _lib.ptr(table), _lib.ptr(offs_d), nf, total, nb, npts,
                int(bool(visible_only)), _lib.ptr(ws), ws.numel(), _lib.ptr(xyz), _lib.ptr(rgb), _lib.ptr(box),
                _lib.ptr(pixel), _lib.ptr(frame_offset), _lib.ptr(kept), _lib.ptr(visible), stream))
            if scores is not None:
                gt_depth, gt_inst, scratch = _score_args(lib, gt, nf, dev)
                _lib.check(lib.mpsr_scene_score(
                    _lib.ptr(xyz_in), _lib.ptr(bf_d), _host(bf), _lib.ptr(scores.box_gt_id), _lib.ptr(gt_depth),
                    _lib.ptr(gt_inst), _lib.ptr(offs_d), nf, total, nb, npts, _lib.ptr(ws), ws.numel(),
                    _lib.ptr(scratch), scratch.numel(), _lib.ptr(scores.counts), _lib.ptr(scores.sums), stream))
            fo_host = frame_offset.cpu().numpy()  # the one copy to the host: M and where each frame's points are
        m = int(fo_host[-1])
    return SceneResult(
        xyz=xyz[:m], rgb=None if rgb is None else rgb[:m], box=box[:m], pixel=pixel[:m], frame_offset=frame_offset,
        depth_maps=_frame_views(depth, hw, offs), instance_maps=_frame_views(inst, hw, offs),
        kept_per_box=kept, visible_per_box=visible, frame_offset_host=fo_host, box_frame_host=bf, scores=scores)


def reconstruct_frames(model, samples, outs, min_score=None, visible_only=False, ground_truth=None, surfaces=None):
    """The scene of a chunk: `samples` as dataset.get_sample_dict returns them, `outs` as model.build_batch returns
    them.  The first num_objs rows of each frame: KEY_INST_XYZ_MAP_LOCAL placed with KEY_VIEW_ANG and KEY_CENTROIDS
    (instance_utils.tf_inst_xyz_map_local_to_global), masked by gt_valid_mask_maps where the sample carries them, kept
    where label_scores >= min_score (None: all), coloured from rgb_image, projected with cam_p.  ground_truth: as
    project_instance_points takes it (box_gt_id over the frames' first num_objs rows, frame after frame).
    surfaces: None, or a dict of render_instance_surfaces' options max_edge_dz and max_span_px ({} for the defaults):
    the same global maps, masks and keep flags are also rendered as surfaces, with the same ground truth, into
    result.surfaces.  -> SceneResult."""
    import torch
    from monopsr_amd.core import constants
    from monopsr_amd.datasets.kitti import instance_utils
    if len(samples) != len(outs):
        raise ValueError('%d samples, %d outputs' % (len(samples), len(outs)))
    if len(samples) == 0:
        raise ValueError('reconstruct_frames needs at least one frame')
    roi = tuple(model.map_roi_size)
    dev = samples[0]['rgb_image'].device
    counts = [int(s['num_objs']) for s in samples]
    with_mask = all(s.get('gt_valid_mask_maps') is not None for s in samples)
    with torch.cuda.device(dev), torch.no_grad():
        cat = lambda ts, tail: torch.cat([t.reshape((n,) + tail) for t, n in zip(ts, counts)], 0)
        local = cat([o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n] for o, n in zip(outs, counts)], roi + (3,))
        view = cat([o[constants.KEY_VIEW_ANG][0:n] for o, n in zip(outs, counts)], (1,))
        cen = cat([o[constants.KEY_CENTROIDS][0:n] for o, n in zip(outs, counts)], (3,))
        glob = instance_utils.tf_inst_xyz_map_local_to_global(local, roi, view, cen)
        mask = cat([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)], roi) if with_mask else None
        keep = None
        if min_score is not None:
            keep = cat([s['label_scores'][0:n] for s, n in zip(samples, counts)], ()) >= float(min_score)
        cam_p = torch.stack([s['cam_p'].reshape(3, 4) for s in samples], 0)
        box_frame = np.repeat(np.arange(len(samples)), counts)
        shapes = [tuple(s['rgb_image'].shape) for s in samples]
        result = project_instance_points(glob, box_frame, cam_p, shapes, images=[s['rgb_image'] for s in samples],
                                         valid_mask=mask, keep=keep, visible_only=visible_only,
                                         ground_truth=ground_truth)
        if surfaces is not None:
            unknown = set(surfaces) - {'max_edge_dz', 'max_span_px'}
            if unknown:
                raise ValueError('surfaces: unknown options %s' % sorted(unknown))
            result.surfaces = render_instance_surfaces(glob, box_frame, cam_p, shapes, valid_mask=mask, keep=keep,
                                                       ground_truth=ground_truth, **surfaces)
        return result


# ---- surfaces


def surface_score_table(counts, sums, box_gt_id):
    """The (B, 6) float32 per-box metric table in SURFACE_METRIC_NAMES order from counts (B, 5) int, sums (B, 3)
    float64 and box_gt_id (B,) int, tensors of one device: computed in fp64, rounded once.
        surface_mask_iou        inter_px / (pred_px + gt_px - inter_px); NaN when the box has no ground truth (id
                                outside [0, 254]) or the union is 0
        surface_mask_precision  inter_px / pred_px; NaN when pred_px == 0
        surface_mask_recall     inter_px / gt_px; NaN when gt_px == 0
        surface_depth_bias      sum e / depth_n          (e = rendered depth - LiDAR depth over the depth_n pixels)
        surface_depth_mae       sum |e| / depth_n
        surface_depth_rmse      sqrt(sum e^2 / depth_n); all three NaN when depth_n == 0"""
    return _metric_table(SURFACE_COUNT_NAMES, ('inter_px', 'gt_px'), counts, sums, box_gt_id)


class SurfaceScores(_Scores):
    """The surfaces against their ground truth, per box, device tensors: counts (B, 5) int32 (SURFACE_COUNT_NAMES),
    sums (B, 3) float64 (SURFACE_SUM_NAMES), box_gt_id (B,) int32 as given.  table(): surface_score_table of them."""
    __slots__ = ()
    _table = staticmethod(surface_score_table)


class FrameSurface(object):
    """One frame of a SurfaceResult: depth_map (h,w) float32, instance_map (h,w) uint8, tri_map (h,w) int32 or None."""
    __slots__ = ('depth_map', 'instance_map', 'tri_map')

    def __init__(self, depth_map, instance_map, tri_map):
        self.depth_map, self.instance_map, self.tri_map = depth_map, instance_map, tri_map


class SurfaceResult(object):
    """What render_instance_surfaces returns, device tensors: depth_maps / instance_maps: lists of (H_f, W_f) float32 /
    uint8 (0 / 255 where no triangle fell); tri_maps: the same of int32 triangle ids (-1: none), or None;
    tris_per_box / pixels_per_box (B,) int32: the triangles a box draws and the pixels it wins; scores: a
    SurfaceScores when the call was given ground truth, else None."""
    __slots__ = ('depth_maps', 'instance_maps', 'tri_maps', 'tris_per_box', 'pixels_per_box', 'scores')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    @property
    def num_frames(self):
        return len(self.depth_maps)

    def frame(self, f):
        return FrameSurface(self.depth_maps[f], self.instance_maps[f], None if self.tri_maps is None else self.tri_maps[f])


def render_instance_surfaces(xyz_global_maps, box_frame, cam_p, frame_shapes, valid_mask=None, keep=None,
                             max_edge_dz=SURFACE_MAX_EDGE_DZ, max_span_px=SURFACE_MAX_SPAN_PX, ground_truth=None,
                             want_tri=False, device=None):
    """The direct wrapper of mpsr_scene_surface_render / _resolve / _score: the boxes' xyz maps rendered as surfaces.

    xyz_global_maps (B, Hm, Wm, 3) float32 CUDA tensor in the camera frame, Hm and Wm 2 or more: neighbouring samples
    are joined into two triangles per grid cell.  box_frame, cam_p, frame_shapes, valid_mask ((B, Hm, Wm[, 1]) or
    (B, Hm Wm)), keep and ground_truth as project_instance_points takes them.  max_edge_dz: a triangle whose three
    depths span more than this many metres is not drawn (it would bridge a depth discontinuity; inf: never);
    max_span_px: nor is one whose pixel extent exceeds this in either direction (1..1024).  want_tri: also return the
    winning triangle id per pixel.  device: where to run (default: the maps' device).  Nothing is copied to the host.
    -> SurfaceResult."""
    import torch
    if not torch.is_tensor(xyz_global_maps) or not xyz_global_maps.is_cuda:
        raise _lib.MpsrError('expected xyz_global_maps on the GPU; monopsr_amd has no CPU path')
    if xyz_global_maps.dim() != 4 or xyz_global_maps.shape[-1] != 3:
        raise _lib.InvalidArgumentError('xyz_global_maps must be (B, Hm, Wm, 3), got %s' % (tuple(xyz_global_maps.shape),))
    dev = xyz_global_maps.device if device is None else torch.device(device)
    nb, mh, mw = (int(v) for v in xyz_global_maps.shape[:3])
    if mh < 2 or mw < 2:
        raise _lib.InvalidArgumentError('a map of %d x %d has no cell (2 x 2 or more)' % (mh, mw))
    max_edge_dz, max_span_px = float(max_edge_dz), int(max_span_px)
    if not max_edge_dz > 0.0:
        raise _lib.InvalidArgumentError('max_edge_dz %r must be greater than 0 (inf: no limit)' % (max_edge_dz,))
    if not 1 <= max_span_px <= 1024:
        raise _lib.InvalidArgumentError('max_span_px %r is outside 1..1024' % (max_span_px,))
    hw, bf, offs = _frame_tables(frame_shapes, box_frame, nb)
    nf = len(hw)
    if nb * (mh - 1) * (mw - 1) * 2 >= 2 ** 32:
        raise _lib.InvalidArgumentError('%d boxes of %d x %d cells: the triangle id does not fit 32 bits'
                                        % (nb, mh - 1, mw - 1))
    total = int(offs[-1])
    lib = _lib.lib()
    i32, f32 = torch.int32, torch.float32
    with torch.cuda.device(dev):
        cam = _cameras(cam_p, nf, dev)
        xyz_in = xyz_global_maps.detach().to(dev).to(f32).contiguous()
        mask, keep_d = _mask_and_keep(valid_mask, keep, nb, mh * mw, dev)
        scores = gt = None
        if ground_truth is not None:
            gt = _ground_truth_tables(ground_truth, hw, nb, dev)
            scores = SurfaceScores(_empty((nb, 5), i32, dev), _empty((nb, 3), torch.float64, dev), gt[2])
        depth = _empty((total,), f32, dev)
        inst = _empty((total,), torch.uint8, dev)
        tri = _empty((total,), i32, dev) if want_tri else None
        if nf == 0 or nb == 0 or total == 0:  # nothing to launch: empty maps
            _fill_empty(depth, inst, scores)
            if tri is not None:
                tri.fill_(-1)
            tris = torch.zeros((nb,), dtype=i32, device=dev)
            pixels = torch.zeros((nb,), dtype=i32, device=dev)
        else:
            hw_d, bf_d, offs_d = _device_tables(hw, bf, offs, dev)
            ws = _empty((lib.mpsr_scene_surface_workspace_bytes(nf, total, nb, mh, mw),), torch.uint8, dev)
            stream = _lib.stream()
            _lib.check(lib.mpsr_scene_surface_render(
                _lib.ptr(xyz_in), _lib.ptr(mask), _lib.ptr(bf_d), _host(bf), _lib.ptr(keep_d), _lib.ptr(cam),
                _lib.ptr(hw_d), _host(hw), _lib.ptr(offs_d), _host(offs), nf, nb, mh, mw, max_edge_dz, max_span_px,
                _lib.ptr(ws), ws.numel(), stream))
            _lib.check(lib.mpsr_scene_surface_resolve(_lib.ptr(bf_d), _host(bf), nf, total, nb, mh, mw, _lib.ptr(ws),
                                                      ws.numel(), _lib.ptr(depth), _lib.ptr(inst), _lib.ptr(tri), stream))
            if scores is None:  # without ground truth: the two per-box counts alone
                counts, sums = _empty((nb, 5), i32, dev), _empty((nb, 3), torch.float64, dev)
                gt_id = gt_depth = gt_inst = scratch = None
            else:
                counts, sums, gt_id = scores.counts, scores.sums, scores.box_gt_id
                gt_depth, gt_inst, scratch = _score_args(lib, gt, nf, dev)
            _lib.check(lib.mpsr_scene_surface_score(
                _lib.ptr(bf_d), _host(bf), _lib.ptr(gt_id), _lib.ptr(gt_depth), _lib.ptr(gt_inst), _lib.ptr(hw_d),
                _lib.ptr(offs_d), nf, total, nb, mh, mw, _lib.ptr(ws), ws.numel(), _lib.ptr(scratch),
                0 if scratch is None else scratch.numel(), _lib.ptr(counts), _lib.ptr(sums), stream))
            tris, pixels = counts[:, 0], counts[:, 1]
    return SurfaceResult(depth_maps=_frame_views(depth, hw, offs), instance_maps=_frame_views(inst, hw, offs),
                         tri_maps=None if tri is None else _frame_views(tri, hw, offs),
                         tris_per_box=tris, pixels_per_box=pixels, scores=scores)


SURFACE_DIRS = ('depth_surface', 'instances_surface')


def _output_dirs(base, kinds):
    dirs = {k: os.path.join(base, k) for k in kinds}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    return dirs


def _host_maps(frame):
    """-> the depth map and the instance map of a FrameScene or a FrameSurface, as arrays."""
    return frame.depth_map.detach().cpu().numpy(), frame.instance_map.detach().cpu().numpy()


def _empty_maps(image_shape):
    """-> the two maps of a frame without a box: depth 0, instance 255 everywhere."""
    h, w = int(image_shape[0]), int(image_shape[1])
    return np.zeros((h, w), np.float32), np.full((h, w), 255, np.uint8)


def _save_maps(out_dirs, kinds, name, depth, inst):
    """<kinds[0]>/<name>.png (depth_map_utils.save_depth_map: uint16, 1/256 m) and <kinds[1]>/<name>.png
    (instance_utils.save_instance_image) of a depth map and an instance map, arrays.  -> the two paths."""
    from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils
    paths = tuple(os.path.join(out_dirs[k], name + '.png') for k in kinds)
    # (a depth beyond the PNG's 16 bits, 256 m, has no place in the format: stored as 0, "no depth")
    depth_map_utils.save_depth_map(paths[0], np.where(depth < 256.0, depth, np.float32(0.0)))
    instance_utils.save_instance_image(paths[1], inst)
    return paths


def surface_output_dirs(base):
    """{'depth_surface' | 'instances_surface': <base>/<kind>}, created."""
    return _output_dirs(base, SURFACE_DIRS)


def save_surface_frame(out_dirs, name, frame_surface):
    """depth_surface/<name>.png and instances_surface/<name>.png of a FrameSurface, in the formats of save_frame's depth
    and instance files.  -> the two paths."""
    return _save_maps(out_dirs, SURFACE_DIRS, name, *_host_maps(frame_surface))


def save_empty_surface_frame(out_dirs, name, image_shape):
    """The two files of a frame without a box: depth 0, instance 255 everywhere.  -> the two paths."""
    return _save_maps(out_dirs, SURFACE_DIRS, name, *_empty_maps(image_shape))


# ---- files


def colours_to_uint8(rgb):
    """float colours -> uchar: clipped to [0, 255], then rounded half to even (254.5 -> 254, 255.5 -> 255, -0.5 -> 0,
    300 -> 255); NaN -> 0."""
    c = np.nan_to_num(np.asarray(rgb, np.float64), nan=0.0)
    return np.rint(np.clip(c, 0.0, 255.0)).astype(np.uint8)


def write_ply(path, xyz, rgb=None, box=None):
    """Binary little-endian PLY of n vertices: float x y z, uchar red green blue, int box.  xyz (n,3); rgb (n,3) float
    (colours_to_uint8) or uint8, None: 0; box (n,) int, None: 0.  n may be 0."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    v = np.zeros(n, _PLY_DTYPE)
    v['x'], v['y'], v['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rgb = np.asarray(rgb)
        c = (rgb if rgb.dtype == np.uint8 else colours_to_uint8(rgb)).reshape(n, 3)
        v['red'], v['green'], v['blue'] = c[:, 0], c[:, 1], c[:, 2]
    if box is not None:
        v['box'] = np.asarray(box).reshape(n)
    with open(path, 'wb') as f:
        f.write((_PLY_HEADER % n).encode('ascii'))
        f.write(v.tobytes())


def read_ply(path):
    """A file of write_ply -> (xyz (n,3) float32, rgb (n,3) uint8, box (n,) int32)."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if end < 0 or not data.startswith(b'ply\n'):
        raise ValueError('%s is not a PLY file' % path)
    header = data[:end + len(b'end_header\n')].decode('ascii')
    n = None
    for line in header.splitlines():
        if line.startswith('element vertex '):
            n = int(line.split()[2])
    if n is None or header != _PLY_HEADER % n:
        raise ValueError('%s: not the header write_ply writes' % path)
    body = data[len(header):]
    if len(body) != n * _PLY_DTYPE.itemsize:
        raise ValueError('%s: %d bytes of vertices, expected %d' % (path, len(body), n * _PLY_DTYPE.itemsize))
    v = np.frombuffer(body, _PLY_DTYPE)
    return (np.stack([v['x'], v['y'], v['z']], 1).astype(np.float32).reshape(n, 3),
            np.stack([v['red'], v['green'], v['blue']], 1).reshape(n, 3), v['box'].astype(np.int32))


SCENE_DIRS = ('points', 'depth', 'instances')


def scene_output_dirs(base):
    """{'points' | 'depth' | 'instances': <base>/<kind>}, created."""
    return _output_dirs(base, SCENE_DIRS)


def save_frame(out_dirs, name, frame_result):
    """points/<name>.ply, depth/<name>.png (depth_map_utils.save_depth_map: uint16, 1/256 m) and instances/<name>.png
    (instance_utils.save_instance_image) of a FrameScene.  -> the three paths."""
    fr = frame_result
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    ply = os.path.join(out_dirs['points'], name + '.ply')
    write_ply(ply, host(fr.xyz), host(fr.rgb), host(fr.box))
    return (ply,) + _save_maps(out_dirs, SCENE_DIRS[1:], name, *_host_maps(fr))


def save_empty_frame(out_dirs, name, image_shape):
    """The three files of a frame without a box (the Evaluator writes an empty label file for it): no vertex, depth 0,
    instance 255 everywhere.  -> the three paths."""
    ply = os.path.join(out_dirs['points'], name + '.ply')
    write_ply(ply, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros(0, np.int32))
    return (ply,) + _save_maps(out_dirs, SCENE_DIRS[1:], name, *_empty_maps(image_shape))
