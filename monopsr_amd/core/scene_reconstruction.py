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

extract_instance_meshes returns the triangles render_instance_surfaces draws as meshes: indexed
faces over the map points they use, with colours, normals and per-box areas; write_mesh_ply writes one frame's as a PLY
file with faces.
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
    reconstruct_frames was asked for it, else None.  meshes: the MeshResult of the same chunk when reconstruct_frames
    was asked for it, else None."""
    __slots__ = ('xyz', 'rgb', 'box', 'pixel', 'frame_offset', 'depth_maps', 'instance_maps', 'kept_per_box',
                 'visible_per_box', 'frame_offset_host', 'box_frame_host', 'scores', 'surfaces', 'meshes')

    def __init__(self, **kw):
        kw.setdefault('scores', None)
        kw.setdefault('surfaces', None)
        kw.setdefault('meshes', None)
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
    result.surfaces.  With 'mesh': True in that dict the drawn triangles are also returned as meshes coloured from
    rgb_image (extract_instance_meshes of the same rendering; 'mesh_visible_only': only the triangles that win a pixel)
    in result.meshes.  -> SceneResult."""
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
            unknown = set(surfaces) - {'max_edge_dz', 'max_span_px', 'mesh', 'mesh_visible_only'}
            if unknown:
                raise ValueError('surfaces: unknown options %s' % sorted(unknown))
            run = _surface_run(glob, box_frame, cam_p, shapes, mask, keep,
                               surfaces.get('max_edge_dz', SURFACE_MAX_EDGE_DZ),
                               surfaces.get('max_span_px', SURFACE_MAX_SPAN_PX), None)
            result.surfaces = _surfaces_of(run, ground_truth, False)
            if surfaces.get('mesh'):  # from the same rendering: one z-buffer serves the maps and the meshes
                result.meshes = _meshes_of(run, [s['rgb_image'] for s in samples],
                                           surfaces.get('mesh_visible_only', False))
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


class _SurfaceRun(object):
    """The checked inputs of a chunk of surfaces on the device and, after render(), the workspace that
    mpsr_scene_surface_render has filled: what render_instance_surfaces and extract_instance_meshes share."""
    __slots__ = ('dev', 'nb', 'mh', 'mw', 'nf', 'total', 'hw', 'bf', 'offs', 'cam', 'xyz_in', 'mask', 'keep',
                 'max_edge_dz', 'max_span_px', 'hw_d', 'bf_d', 'offs_d', 'ws', 'stream')

    @property
    def empty(self):
        """Nothing to launch?"""
        return self.nf == 0 or self.nb == 0 or self.total == 0

    def render(self):
        """The device tables, the workspace and mpsr_scene_surface_render (once; not for an empty chunk)."""
        import torch
        if self.ws is not None:
            return
        lib = _lib.lib()
        self.hw_d, self.bf_d, self.offs_d = _device_tables(self.hw, self.bf, self.offs, self.dev)
        self.ws = _empty((lib.mpsr_scene_surface_workspace_bytes(self.nf, self.total, self.nb, self.mh, self.mw),),
                         torch.uint8, self.dev)
        self.stream = _lib.stream()
        _lib.check(lib.mpsr_scene_surface_render(
            _lib.ptr(self.xyz_in), _lib.ptr(self.mask), _lib.ptr(self.bf_d), _host(self.bf), _lib.ptr(self.keep),
            _lib.ptr(self.cam), _lib.ptr(self.hw_d), _host(self.hw), _lib.ptr(self.offs_d), _host(self.offs), self.nf,
            self.nb, self.mh, self.mw, self.max_edge_dz, self.max_span_px, _lib.ptr(self.ws), self.ws.numel(),
            self.stream))


def _surface_run(xyz_global_maps, box_frame, cam_p, frame_shapes, valid_mask, keep, max_edge_dz, max_span_px, device):
    """The arguments render_instance_surfaces and extract_instance_meshes share, checked and moved to the device.
    -> _SurfaceRun, nothing launched yet."""
    import torch
    if not torch.is_tensor(xyz_global_maps) or not xyz_global_maps.is_cuda:
        raise _lib.MpsrError('expected xyz_global_maps on the GPU; monopsr_amd has no CPU path')
    if xyz_global_maps.dim() != 4 or xyz_global_maps.shape[-1] != 3:
        raise _lib.InvalidArgumentError('xyz_global_maps must be (B, Hm, Wm, 3), got %s' % (tuple(xyz_global_maps.shape),))
    run = _SurfaceRun()
    run.dev = dev = xyz_global_maps.device if device is None else torch.device(device)
    run.nb, run.mh, run.mw = nb, mh, mw = tuple(int(v) for v in xyz_global_maps.shape[:3])
    if mh < 2 or mw < 2:
        raise _lib.InvalidArgumentError('a map of %d x %d has no cell (2 x 2 or more)' % (mh, mw))
    run.max_edge_dz, run.max_span_px = max_edge_dz, max_span_px = float(max_edge_dz), int(max_span_px)
    if not max_edge_dz > 0.0:
        raise _lib.InvalidArgumentError('max_edge_dz %r must be greater than 0 (inf: no limit)' % (max_edge_dz,))
    if not 1 <= max_span_px <= 1024:
        raise _lib.InvalidArgumentError('max_span_px %r is outside 1..1024' % (max_span_px,))
    run.hw, run.bf, run.offs = _frame_tables(frame_shapes, box_frame, nb)
    run.nf = len(run.hw)
    if nb * (mh - 1) * (mw - 1) * 2 >= 2 ** 32:
        raise _lib.InvalidArgumentError('%d boxes of %d x %d cells: the triangle id does not fit 32 bits'
                                        % (nb, mh - 1, mw - 1))
    run.total = int(run.offs[-1])
    run.hw_d = run.bf_d = run.offs_d = run.ws = run.stream = None
    with torch.cuda.device(dev):
        run.cam = _cameras(cam_p, run.nf, dev)
        run.xyz_in = xyz_global_maps.detach().to(dev).to(torch.float32).contiguous()
        run.mask, run.keep = _mask_and_keep(valid_mask, keep, nb, mh * mw, dev)
    return run


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
    return _surfaces_of(_surface_run(xyz_global_maps, box_frame, cam_p, frame_shapes, valid_mask, keep, max_edge_dz,
                                     max_span_px, device), ground_truth, want_tri)


def _surfaces_of(run, ground_truth, want_tri):
    """render_instance_surfaces of a _SurfaceRun."""
    import torch
    dev, nb, mh, mw, nf, total, hw, bf, offs = (run.dev, run.nb, run.mh, run.mw, run.nf, run.total, run.hw, run.bf,
                                                run.offs)
    lib = _lib.lib()
    i32, f32 = torch.int32, torch.float32
    with torch.cuda.device(dev):
        scores = gt = None
        if ground_truth is not None:
            gt = _ground_truth_tables(ground_truth, hw, nb, dev)
            scores = SurfaceScores(_empty((nb, 5), i32, dev), _empty((nb, 3), torch.float64, dev), gt[2])
        depth = _empty((total,), f32, dev)
        inst = _empty((total,), torch.uint8, dev)
        tri = _empty((total,), i32, dev) if want_tri else None
        if run.empty:  # nothing to launch: empty maps
            _fill_empty(depth, inst, scores)
            if tri is not None:
                tri.fill_(-1)
            tris = torch.zeros((nb,), dtype=i32, device=dev)
            pixels = torch.zeros((nb,), dtype=i32, device=dev)
        else:
            run.render()
            bf_d, hw_d, offs_d, ws, stream = run.bf_d, run.hw_d, run.offs_d, run.ws, run.stream
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


# ---- meshes


class FrameMesh(object):
    """One frame of a MeshResult, a mesh of its own: xyz, rgb, normal (v,3) float32, box (v,) int32 and face_box (t,)
    int32 = the ordinal within the frame (the value of the instance image), faces (t,3) int32 indices into this
    frame's vertices, area_per_box (n,) float64 of the frame's boxes."""
    __slots__ = ('xyz', 'rgb', 'normal', 'box', 'faces', 'face_box', 'area_per_box')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


class MeshResult(object):
    """What extract_instance_meshes returns, device tensors: xyz, rgb, normal (V,3) float32, vertex_box (V,) int32
    (index into the call's boxes), faces (T,3) int32 = FRAME-LOCAL vertex indices in the order (a, c, b) (counter-
    clockwise seen from the camera), face_box (T,) int32, area_per_box (B,) float64 (square metres),
    vertex_box_offset / face_box_offset (B+1,) and vertex_frame_offset / face_frame_offset (F+1,) int64: box b owns
    rows box_offset[b] .. box_offset[b+1], frame f rows frame_offset[f] .. frame_offset[f+1].  *_host are the host
    copies of the two frame tables and of box_frame."""
    __slots__ = ('xyz', 'rgb', 'normal', 'vertex_box', 'faces', 'face_box', 'area_per_box', 'vertex_box_offset',
                 'vertex_frame_offset', 'face_box_offset', 'face_frame_offset', 'vertex_frame_offset_host',
                 'face_frame_offset_host', 'box_frame_host')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    @property
    def num_frames(self):
        return len(self.vertex_frame_offset_host) - 1

    def frame(self, f):
        v0, v1 = int(self.vertex_frame_offset_host[f]), int(self.vertex_frame_offset_host[f + 1])
        t0, t1 = int(self.face_frame_offset_host[f]), int(self.face_frame_offset_host[f + 1])
        b0, b1 = (int(v) for v in np.searchsorted(self.box_frame_host, [f, f + 1]))
        return FrameMesh(xyz=self.xyz[v0:v1], rgb=self.rgb[v0:v1], normal=self.normal[v0:v1],
                         box=self.vertex_box[v0:v1] - b0, faces=self.faces[t0:t1], face_box=self.face_box[t0:t1] - b0,
                         area_per_box=self.area_per_box[b0:b1])


def extract_instance_meshes(xyz_global_maps, box_frame, cam_p, frame_shapes, valid_mask=None, keep=None, images=None,
                            max_edge_dz=SURFACE_MAX_EDGE_DZ, max_span_px=SURFACE_MAX_SPAN_PX, visible_only=False,
                            device=None):
    """The direct wrapper of mpsr_scene_surface_render followed by mpsr_scene_surface_mesh: the triangles
    render_instance_surfaces draws, as indexed faces over the map points they use.

    The arguments of render_instance_surfaces; images None or F CUDA tensors (h_f, w_f, 3) float32 as
    project_instance_points takes them: a vertex has the colour of the pixel it projects to, (0, 0, 0) outside the
    frame or without images.  visible_only: only the triangles that win at least one pixel of the z-buffer.  One copy
    of the two (F + 1) frame offset tables to the host tells how many vertices and faces there are.  -> MeshResult."""
    return _meshes_of(_surface_run(xyz_global_maps, box_frame, cam_p, frame_shapes, valid_mask, keep, max_edge_dz,
                                   max_span_px, device), images, visible_only)


def _meshes_of(run, images, visible_only):
    """extract_instance_meshes of a _SurfaceRun."""
    import torch
    dev, nb, mh, mw, nf, hw = run.dev, run.nb, run.mh, run.mw, run.nf, run.hw
    if images is not None and len(images) != nf:
        raise _lib.InvalidArgumentError('%d images for %d frames' % (len(images), nf))
    if nb * mh * mw >= 2 ** 31:
        raise _lib.InvalidArgumentError('%d boxes of %d x %d points: a vertex index does not fit 31 bits' % (nb, mh, mw))
    lib = _lib.lib()
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    with torch.cuda.device(dev):
        table, imgs = None, []
        if images is not None:
            for f, im in enumerate(images):
                if not torch.is_tensor(im) or tuple(im.shape) != (int(hw[f, 0]), int(hw[f, 1]), 3):
                    raise _lib.InvalidArgumentError('image %d must be a (%d, %d, 3) tensor' % (f, hw[f, 0], hw[f, 1]))
                imgs.append(im.detach().to(dev).to(f32).contiguous())  # (kept alive until the launches are queued)
            table = torch.from_numpy(np.asarray([_lib.ptr(im) for im in imgs] or [0], np.uint64).view(np.int64)).to(dev)
        v_cap, t_cap = nb * mh * mw, nb * 2 * (mh - 1) * (mw - 1)
        xyz, rgb, normal = (_empty((v_cap, 3), f32, dev) for _ in range(3))
        vertex_box = _empty((v_cap,), i32, dev)
        faces, face_box = _empty((t_cap, 3), i32, dev), _empty((t_cap,), i32, dev)
        area = _empty((nb,), torch.float64, dev)
        # one buffer for the four tables: [vertex frames | face frames | vertex boxes | face boxes], so that ONE copy
        # brings both frame tables to the host
        offsets = _empty((2 * (nf + 1) + 2 * (nb + 1),), i64, dev)
        v_frame, t_frame = offsets[:nf + 1], offsets[nf + 1:2 * (nf + 1)]
        v_box, t_box = offsets[2 * (nf + 1):2 * (nf + 1) + nb + 1], offsets[2 * (nf + 1) + nb + 1:]
        if run.empty:  # nothing to launch: no vertex, no face
            offsets.zero_()
            area.zero_()
            host = np.zeros(2 * (nf + 1), np.int64)
        else:
            run.render()
            ws = _empty((lib.mpsr_scene_surface_mesh_workspace_bytes(nb, mh, mw),), torch.uint8, dev)
            _lib.check(lib.mpsr_scene_surface_mesh(
                _lib.ptr(run.xyz_in), _lib.ptr(run.bf_d), _host(run.bf), _lib.ptr(run.cam), _lib.ptr(run.hw_d),
                _host(run.hw), _lib.ptr(run.offs_d), _host(run.offs), _lib.ptr(table), nf, nb, mh, mw, run.max_edge_dz,
                run.max_span_px, int(bool(visible_only)), _lib.ptr(run.ws), run.ws.numel(), _lib.ptr(ws), ws.numel(),
                _lib.ptr(xyz), _lib.ptr(rgb), _lib.ptr(normal), _lib.ptr(vertex_box), _lib.ptr(faces),
                _lib.ptr(face_box), _lib.ptr(area), v_box.data_ptr(), v_frame.data_ptr(), t_box.data_ptr(),
                t_frame.data_ptr(), run.stream))
            host = offsets[:2 * (nf + 1)].cpu().numpy()  # the one copy to the host: V, T and where each frame's are
        v_host, t_host = host[:nf + 1], host[nf + 1:]
        nv, nt = int(v_host[-1]), int(t_host[-1])
    return MeshResult(xyz=xyz[:nv], rgb=rgb[:nv], normal=normal[:nv], vertex_box=vertex_box[:nv], faces=faces[:nt],
                      face_box=face_box[:nt], area_per_box=area, vertex_box_offset=v_box, vertex_frame_offset=v_frame,
                      face_box_offset=t_box, face_frame_offset=t_frame, vertex_frame_offset_host=v_host,
                      face_frame_offset_host=t_host, box_frame_host=run.bf)


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


# ---- mesh files

_MESH_VERTEX_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'),
                               ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('box', '<i4')])
_MESH_FACE_DTYPE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
_MESH_HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n'
                'property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n'
                'property uchar green\nproperty uchar blue\nproperty int box\nelement face %d\n'
                'property list uchar int vertex_indices\nend_header\n')


def write_mesh_ply(path, xyz, faces, rgb=None, normal=None, box=None):
    """Binary little-endian PLY of n vertices (float x y z, float nx ny nz, uchar red green blue, int box) and t
    triangles (list uchar int vertex_indices): what MeshLab and CloudCompare open.  xyz (n,3); faces (t,3) ints in
    [0, n); rgb (n,3) float (colours_to_uint8) or uint8, None: 0; normal (n,3), None: 0; box (n,) int, None: 0.  n and
    t may be 0."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    n = len(xyz)
    if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= n):
        raise ValueError('faces index vertices outside [0, %d)' % n)
    v = np.zeros(n, _MESH_VERTEX_DTYPE)
    v['x'], v['y'], v['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normal is not None:
        normal = np.asarray(normal, np.float32).reshape(n, 3)
        v['nx'], v['ny'], v['nz'] = normal[:, 0], normal[:, 1], normal[:, 2]
    if rgb is not None:
        rgb = np.asarray(rgb)
        c = (rgb if rgb.dtype == np.uint8 else colours_to_uint8(rgb)).reshape(n, 3)
        v['red'], v['green'], v['blue'] = c[:, 0], c[:, 1], c[:, 2]
    if box is not None:
        v['box'] = np.asarray(box).reshape(n)
    t = np.zeros(len(faces), _MESH_FACE_DTYPE)
    t['n'] = 3
    t['v'] = faces
    with open(path, 'wb') as f:
        f.write((_MESH_HEADER % (n, len(faces))).encode('ascii'))
        f.write(v.tobytes())
        f.write(t.tobytes())


def read_mesh_ply(path):
    """A file of write_mesh_ply -> (xyz (n,3) float32, faces (t,3) int32, rgb (n,3) uint8, normal (n,3) float32, box
    (n,) int32)."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if end < 0 or not data.startswith(b'ply\n'):
        raise ValueError('%s is not a PLY file' % path)
    header = data[:end + len(b'end_header\n')].decode('ascii')
    count = {}
    for line in header.splitlines():
        if line.startswith('element '):
            count[line.split()[1]] = int(line.split()[2])
    if set(count) != {'vertex', 'face'} or header != _MESH_HEADER % (count['vertex'], count['face']):
        raise ValueError('%s: not the header write_mesh_ply writes' % path)
    n, t = count['vertex'], count['face']
    body = data[len(header):]
    want = n * _MESH_VERTEX_DTYPE.itemsize + t * _MESH_FACE_DTYPE.itemsize
    if len(body) != want:
        raise ValueError('%s: %d bytes of vertices and faces, expected %d' % (path, len(body), want))
    v = np.frombuffer(body, _MESH_VERTEX_DTYPE, n)
    faces = np.frombuffer(body, _MESH_FACE_DTYPE, t, n * _MESH_VERTEX_DTYPE.itemsize)
    if t and not bool((faces['n'] == 3).all()):
        raise ValueError('%s: a face is not a triangle' % path)
    return (np.stack([v['x'], v['y'], v['z']], 1).astype(np.float32).reshape(n, 3),
            faces['v'].astype(np.int32).reshape(t, 3), np.stack([v['red'], v['green'], v['blue']], 1).reshape(n, 3),
            np.stack([v['nx'], v['ny'], v['nz']], 1).astype(np.float32).reshape(n, 3), v['box'].astype(np.int32))


MESH_DIRS = ('mesh',)


def mesh_output_dirs(base):
    """{'mesh': <base>/mesh}, created."""
    return _output_dirs(base, MESH_DIRS)


def save_mesh_frame(out_dirs, name, frame_mesh):
    """mesh/<name>.ply of a FrameMesh.  -> the path."""
    fm = frame_mesh
    host = lambda t: t.detach().cpu().numpy()
    ply = os.path.join(out_dirs['mesh'], name + '.ply')
    write_mesh_ply(ply, host(fm.xyz), host(fm.faces), host(fm.rgb), host(fm.normal), host(fm.box))
    return ply


def save_empty_mesh_frame(out_dirs, name):
    """The file of a frame without a box: 0 vertices, 0 faces.  -> the path."""
    ply = os.path.join(out_dirs['mesh'], name + '.ply')
    write_mesh_ply(ply, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    return ply
