"""Instance-map geometry, mirroring the TF functions of the reference's datasets/kitti/instance_utils.py that sit on
the model's output path (same names and argument meaning).  Tensors are torch CUDA tensors; the compute is
libmonopsr_hip.so (geometry.hip), wrapped in autograd Functions so the training loss can differentiate through it.

The training ground truth comes from the same module (instance_maps.hip):

    images = gen_instance_images(depth_maps, calibs, labels_per_frame)      # (F, H, W) uint8 CUDA tensor
    save_instance_image(path, images[0].cpu().numpy())
    local, glob, valid = instance_xyz_crops(depth_maps, images, p2s, frame_index, instance_id, boxes_2d, boxes_3d,
                                            view_angs, roi=(48, 48))

Command line (what demos/instances/gen_instance_masks.py does for a split directory with label_2/, calib/, image_2/
and a directory of depth maps):

    python -m monopsr_amd.datasets.kitti.instance_utils SPLIT_DIR DEPTH_DIR OUT_DIR [--frames 000001 ...] [--batch 8]

writes OUT_DIR/<name>.png, 255 on the background and k on the k-th kept label.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

from monopsr_amd import _lib


def _f32(t):
    return t.contiguous().float()


class _XyzLocalToGlobal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_local, view_angs, centroids):
        n = xyz_local.shape[0]
        p = xyz_local[0].numel() // 3 if n else 0
        xyz_local, view_angs, centroids = _f32(xyz_local), _f32(view_angs).reshape(-1), _f32(centroids)
        out = torch.empty_like(xyz_local)
        _lib.check(_lib.lib().mpsr_xyz_map_local_to_global(_lib.ptr(xyz_local), _lib.ptr(view_angs),
                                                           _lib.ptr(centroids), _lib.ptr(out), n, p, _lib.stream()))
        ctx.save_for_backward(view_angs)
        ctx.dims = (n, p)
        return out

    @staticmethod
    def backward(ctx, g):
        (view_angs,) = ctx.saved_tensors
        n, p = ctx.dims
        g = _f32(g)
        need_local, _, need_cen = ctx.needs_input_grad
        gl = torch.empty_like(g) if need_local else None
        gc = torch.empty((n, 3), dtype=torch.float32, device=g.device) if need_cen else None
        if need_local or need_cen:
            _lib.check(_lib.lib().mpsr_xyz_map_local_to_global_grad(_lib.ptr(g), _lib.ptr(view_angs), _lib.ptr(gl),
                                                                    _lib.ptr(gc), n, p, _lib.stream()))
        return gl, None, gc  # the viewing angle is an input of the graph (view_ang: 'est'), never a variable


def tf_inst_xyz_map_local_to_global(inst_xyz_map_local, map_roi_size, view_angs, centroids):
    """instance_utils.py:567-602.  (N,H,W,3) local map, (N,1) viewing angles, (N,3) centroids -> (N,H,W,3):
    every point rotated about y by the viewing angle, then translated by the centroid."""
    if inst_xyz_map_local.dim() != 4 or inst_xyz_map_local.shape[3] != 3:
        raise _lib.InvalidArgumentError("inst_xyz_map_local must be (N, H, W, 3)")
    n = inst_xyz_map_local.shape[0]
    if tuple(inst_xyz_map_local.shape[1:3]) != tuple(map_roi_size):
        raise _lib.InvalidArgumentError("inst_xyz_map_local does not match map_roi_size %s" % (tuple(map_roi_size),))
    if view_angs.numel() != n or tuple(centroids.shape) != (n, 3):
        raise _lib.InvalidArgumentError("view_angs must be (N, 1) and centroids (N, 3)")
    return _XyzLocalToGlobal.apply(inst_xyz_map_local, view_angs, centroids)


def _cam_index(cam_index):
    return None if cam_index is None else cam_index.reshape(-1).to(torch.int32).contiguous()


def _check_cams(cam_p, cam_index, n):
    """cam_p (3,4) without an index, (n_cams,3,4) with cam_index (n)."""
    if cam_index is None:
        if cam_p.numel() != 12:
            raise _lib.InvalidArgumentError("cam_p must be (3,4); per-box cameras (n_cams,3,4) need cam_index")
    elif cam_p.numel() == 0 or cam_p.numel() % 12 or cam_index.numel() != n:
        raise _lib.InvalidArgumentError("per-box cameras: cam_p must be (n_cams,3,4) and cam_index (N)")


class _DepthLocalToGlobal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_local, global_depth, box_2d, inst_view_ang, cam_p, rotate_view, cam_index=None):
        n, h, w = depth_local.shape[:3]
        # a (N,H,W,1) slice of an xyz map is read in place through its channel stride
        if depth_local.dim() == 4 and depth_local.stride(3) == 1 and depth_local.stride(2) > 1 and \
                depth_local.stride(1) == w * depth_local.stride(2) and depth_local.stride(0) == h * depth_local.stride(1) \
                and depth_local.dtype == torch.float32:
            src, stride = depth_local, depth_local.stride(2)
        else:
            src, stride = _f32(depth_local), 1
        z = _f32(global_depth).reshape(-1)
        out = torch.empty((n, h, w, 1), dtype=torch.float32, device=depth_local.device)
        boxes = _f32(box_2d) if rotate_view else None
        va = _f32(inst_view_ang).reshape(-1) if rotate_view else None
        cam = _f32(cam_p).reshape(-1) if rotate_view else None
        idx = _cam_index(cam_index) if rotate_view else None
        if idx is None:
            _lib.check(_lib.lib().mpsr_depth_map_local_to_global(src.data_ptr(), stride, _lib.ptr(z), _lib.ptr(boxes),
                                                                 _lib.ptr(va), _lib.ptr(cam), _lib.ptr(out), n, h, w,
                                                                 int(bool(rotate_view)), _lib.stream()))
        else:
            _lib.check(_lib.lib().mpsr_depth_map_local_to_global_cams(
                src.data_ptr(), stride, _lib.ptr(z), _lib.ptr(boxes), _lib.ptr(va), _lib.ptr(cam), cam.numel() // 12,
                _lib.ptr(idx), _lib.ptr(out), n, h, w, 1, _lib.stream()))
        ctx.save_for_backward(*(t for t in (boxes, va, cam, idx) if t is not None))
        ctx.meta = (n, h, w, bool(rotate_view), tuple(global_depth.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        n, h, w, rotate, zshape = ctx.meta
        boxes, va, cam, idx = (tuple(ctx.saved_tensors) + (None,))[:4] if rotate else (None, None, None, None)
        g = _f32(g)
        gz = None
        if ctx.needs_input_grad[1]:
            gz = torch.empty((n,), dtype=torch.float32, device=g.device)
            if idx is None:
                _lib.check(_lib.lib().mpsr_depth_map_local_to_global_grad(_lib.ptr(g), _lib.ptr(boxes), _lib.ptr(va),
                                                                          _lib.ptr(cam), _lib.ptr(gz), n, h, w,
                                                                          int(rotate), _lib.stream()))
            else:
                _lib.check(_lib.lib().mpsr_depth_map_local_to_global_grad_cams(
                    _lib.ptr(g), _lib.ptr(boxes), _lib.ptr(va), _lib.ptr(cam), cam.numel() // 12, _lib.ptr(idx),
                    _lib.ptr(gz), n, h, w, 1, _lib.stream()))
            gz = gz.reshape(zshape)
        return (g if ctx.needs_input_grad[0] else None), gz, None, None, None, None, None


def tf_inst_depth_map_local_to_global(inst_depth_map_local, global_depth, box_2d=None, inst_view_ang=None,
                                      map_roi_size=None, cam_p=None, rotate_view=False, cam_index=None):
    """instance_utils.py:605-680.  (N,H,W,1) local depth + (N,1) centroid depth -> (N,H,W,1) global depth; with
    rotate_view the view-normalisation offset is added (interpolated between the box's edge rays with H samples
    and laid out along the ROW axis, exactly as the reference does).
    cam_index (N) int32 with cam_p (n_cams,3,4): the boxes of several frames, each with its frame's camera
    (mpsr_depth_map_local_to_global_cams); without it cam_p is one (3,4) matrix, as in the reference."""
    if inst_depth_map_local.dim() != 4 or inst_depth_map_local.shape[3] != 1:
        raise _lib.InvalidArgumentError("inst_depth_map_local must be (N, H, W, 1)")
    if rotate_view and (box_2d is None or inst_view_ang is None or cam_p is None):
        raise _lib.InvalidArgumentError("rotate_view needs box_2d, inst_view_ang and cam_p")
    if map_roi_size is not None and tuple(inst_depth_map_local.shape[1:3]) != tuple(map_roi_size):
        raise _lib.InvalidArgumentError("inst_depth_map_local does not match map_roi_size")
    if rotate_view:
        _check_cams(cam_p, cam_index, inst_depth_map_local.shape[0])
    return _DepthLocalToGlobal.apply(inst_depth_map_local, global_depth, box_2d, inst_view_ang, cam_p, rotate_view,
                                     cam_index)


class _ProjErrNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_global, boxes_2d, cam_p, valid_mask, want_maps, cam_index=None):
        n, h, w = xyz_global.shape[:3]
        xyz_global, boxes_2d = _f32(xyz_global), _f32(boxes_2d)
        cam_p, valid_mask = _f32(cam_p).reshape(-1), _f32(valid_mask).reshape(n, h, w)
        norm = torch.empty((n,), dtype=torch.float32, device=xyz_global.device)
        maps = torch.empty((n, h, w, 2), dtype=torch.float32, device=xyz_global.device) if want_maps else None
        idx = _cam_index(cam_index)
        if idx is None:
            _lib.check(_lib.lib().mpsr_proj_err_norm(_lib.ptr(xyz_global), _lib.ptr(boxes_2d), _lib.ptr(cam_p),
                                                     _lib.ptr(valid_mask), _lib.ptr(maps), _lib.ptr(norm), n, h, w,
                                                     _lib.stream()))
            ctx.save_for_backward(xyz_global, boxes_2d, cam_p, valid_mask)
        else:
            _lib.check(_lib.lib().mpsr_proj_err_norm_cams(_lib.ptr(xyz_global), _lib.ptr(boxes_2d), _lib.ptr(cam_p),
                                                          cam_p.numel() // 12, _lib.ptr(idx), _lib.ptr(valid_mask),
                                                          _lib.ptr(maps), _lib.ptr(norm), n, h, w, _lib.stream()))
            ctx.save_for_backward(xyz_global, boxes_2d, cam_p, valid_mask, idx)
        if maps is None:
            maps = norm.new_empty(0)
        ctx.mark_non_differentiable(maps)
        return norm, maps

    @staticmethod
    def backward(ctx, gnorm, _gmaps):
        xyz_global, boxes_2d, cam_p, valid_mask, idx = (tuple(ctx.saved_tensors) + (None,))[:5]
        n, h, w = xyz_global.shape[:3]
        gx = torch.empty_like(xyz_global)
        if idx is None:
            _lib.check(_lib.lib().mpsr_proj_err_norm_grad(_lib.ptr(_f32(gnorm)), _lib.ptr(xyz_global),
                                                          _lib.ptr(boxes_2d), _lib.ptr(cam_p), _lib.ptr(valid_mask),
                                                          _lib.ptr(gx), n, h, w, _lib.stream()))
        else:
            _lib.check(_lib.lib().mpsr_proj_err_norm_grad_cams(
                _lib.ptr(_f32(gnorm)), _lib.ptr(xyz_global), _lib.ptr(boxes_2d), _lib.ptr(cam_p), cam_p.numel() // 12,
                _lib.ptr(idx), _lib.ptr(valid_mask), _lib.ptr(gx), n, h, w, _lib.stream()))
        return gx, None, None, None, None, None


def proj_err_maps_norm(pred_inst_xyz_map_global, pred_boxes_2d, cam_p, valid_mask_maps, want_maps=False,
                       cam_index=None):
    """The arithmetic of monopsr_output_builder.py:681-746 (get_proj_err_maps_norm) -> (proj_err_norm (N,),
    proj_err_maps_norm (N,H,W,2) or None).  Differentiable w.r.t. the global map.
    cam_index (N) int32 with cam_p (n_cams,3,4): each box projected with its own frame's camera
    (mpsr_proj_err_norm_cams); without it cam_p is one (3,4) matrix, as in the reference."""
    if pred_inst_xyz_map_global.dim() != 4 or pred_inst_xyz_map_global.shape[3] != 3:
        raise _lib.InvalidArgumentError("pred_inst_xyz_map_global must be (N, H, W, 3)")
    n = pred_inst_xyz_map_global.shape[0]
    if tuple(pred_boxes_2d.shape) != (n, 4) or (cam_index is None and cam_p.numel() != 12) or \
            valid_mask_maps.numel() != pred_inst_xyz_map_global.numel() // 3:
        raise _lib.InvalidArgumentError("boxes_2d must be (N,4), cam_p (3,4), valid_mask_maps (N,H,W,1)")
    _check_cams(cam_p, cam_index, n)
    norm, maps = _ProjErrNorm.apply(pred_inst_xyz_map_global, pred_boxes_2d, cam_p, valid_mask_maps, want_maps,
                                    cam_index)
    return norm, (maps if want_maps else None)


def format_boxes(lwh, view_angs, alpha_bins, alpha_regs, centroids, boxes_2d, scores, class_indices, cam_p,
                 img_shape, centroid_type='middle', post_process_cen_x=True, max_depth=45.0):
    """monopsr_model.py:960-1071 format_predictions' box arithmetic, incl. postprocess_cen_x
    (instance_utils.py:988-1032) and score_boxes (monopsr_output_builder.py:805-860), on the device in fp64:
    -> (box_3d (N,9) [x,y,z,l,w,h,ry,score,class-1], box_2d (N,7) [y1,x1,y2,x2,alpha,score,class-1])."""
    n, nb = alpha_bins.shape
    dev = alpha_bins.device
    b3 = torch.empty((n, 9), dtype=torch.float32, device=dev)
    b2 = torch.empty((n, 7), dtype=torch.float32, device=dev)
    args = [_f32(t) for t in (lwh, view_angs.reshape(-1), alpha_bins, alpha_regs, centroids, boxes_2d,
                              scores.reshape(-1))]
    cls = class_indices.reshape(-1).contiguous().int()
    cam = _f32(cam_p).reshape(-1)
    _lib.check(_lib.lib().mpsr_format_boxes(*[_lib.ptr(t) for t in args], _lib.ptr(cls), _lib.ptr(cam), n, nb,
                                            int(img_shape[0]), int(img_shape[1]), int(centroid_type == 'middle'),
                                            int(bool(post_process_cen_x)), float(max_depth), _lib.ptr(b3),
                                            _lib.ptr(b2), _lib.stream()))
    return b3, b2


# ------------------------------------------------------------------------------ placing a cloud on its viewing ray

def get_exp_proj_uv_map(boxes_2d, roi_size, round_box_2d=False, use_pixel_centres=False):
    """instance_utils.py:684-735 for N boxes: (N,4) [y1,x1,y2,x2] -> (N,H,W,2) expected [u, v] of an evenly spaced
    roi_size grid over each box, on the boxes' device: the pixels' top-left corners, or their centres with
    use_pixel_centres.  np.linspace's start + index * step in float32, the arithmetic of mpsr_proj_points."""
    h, w = int(roi_size[0]), int(roi_size[1])
    b = _f32(boxes_2d).reshape(-1, 4)
    if round_box_2d:
        b = torch.round(b)  # half to even, as np.round
    v1, u1, v2, u2 = b[:, 0:1], b[:, 1:2], b[:, 2:3], b[:, 3:4]
    su, sv = (u2 - u1) / w, (v2 - v1) / h
    if use_pixel_centres:
        u0, ue, v0, ve = u1 + su / 2.0, u2 - su / 2.0, v1 + sv / 2.0, v2 - sv / 2.0
    else:
        u0, ue, v0, ve = u1, u2 - su, v1, v2 - sv
    du = (ue - u0) / (w - 1) if w > 1 else torch.zeros_like(u0)
    dv = (ve - v0) / (h - 1) if h > 1 else torch.zeros_like(v0)
    grid_u = u0 + du * torch.arange(w, dtype=torch.float32, device=b.device)[None]
    grid_v = v0 + dv * torch.arange(h, dtype=torch.float32, device=b.device)[None]
    return torch.stack([grid_u[:, None, :].expand(-1, h, w), grid_v[:, :, None].expand(-1, h, w)], 3).contiguous()


def _placement(xz_dist, centroid_y, viewing_angle, n):
    """-> x (n,3) float32 [xz_dist, centroid_y, viewing_angle]"""
    cols = [_f32(torch.as_tensor(t)).reshape(-1) for t in (xz_dist, centroid_y, viewing_angle)]
    if any(c.numel() != n for c in cols):
        raise _lib.InvalidArgumentError("xz_dist, centroid_y and viewing_angle must have one entry per box (%d)" % n)
    return torch.stack(cols, 1).contiguous()


def proj_points_err(x, inst_points_local, boxes_2d, cam_p, roi_size, valid_mask=None, rotate_view=True,
                    cam0_shift=True, round_box_2d=False, use_pixel_centres=False, cam_index=None, want_points=True):
    """The direct wrapper of mpsr_proj_points: x (N,3) [xz_dist, centroid_y, viewing_angle], local points (N,P,3) in map
    order, boxes (N,4) -> (points_uv (N,2,P) float32, valid (N,P) bool, err (N,) float64); the first two None without
    want_points."""
    n = int(inst_points_local.shape[0])
    h, w = int(roi_size[0]), int(roi_size[1])
    if inst_points_local.numel() != n * h * w * 3:
        raise _lib.InvalidArgumentError("inst_points_local %s does not hold %d x %d points per box"
                                        % (tuple(inst_points_local.shape), h, w))
    local = _f32(inst_points_local).reshape(n, h * w, 3)
    if tuple(x.shape) != (n, 3) or tuple(boxes_2d.shape) != (n, 4):
        raise _lib.InvalidArgumentError("x must be (N,3) and boxes_2d (N,4)")
    if valid_mask is not None and valid_mask.numel() != n * h * w:
        raise _lib.InvalidArgumentError("valid_mask must hold one entry per point")
    _check_cams(cam_p, cam_index, n)
    dev = local.device
    x, boxes, cam, idx = _f32(x), _f32(boxes_2d), _f32(cam_p).reshape(-1), _cam_index(cam_index)
    mask = None if valid_mask is None else _f32(valid_mask).reshape(n, h * w)
    uv = torch.empty((n, 2, h * w), dtype=torch.float32, device=dev) if want_points else None
    valid = torch.empty((n, h * w), dtype=torch.uint8, device=dev) if want_points else None
    err = torch.empty((n,), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().mpsr_proj_points(
        _lib.ptr(local), _lib.ptr(x), _lib.ptr(boxes), _lib.ptr(cam), cam.numel() // 12, _lib.ptr(idx), _lib.ptr(mask),
        _lib.ptr(uv), _lib.ptr(valid), _lib.ptr(err), n, h, w, int(bool(rotate_view)), int(bool(cam0_shift)),
        int(bool(round_box_2d)), int(bool(use_pixel_centres)), _lib.stream()))
    return uv, (valid.bool() if want_points else None), err


def proj_points(xz_dist, centroid_y, viewing_angle, inst_points_local, cam_p, rotate_view=True, cam0_shift=True,
                cam_index=None):
    """instance_utils.py:791-838, batched over boxes: (N,) distances along the viewing ray, heights and viewing angles,
    (N,P,3) local points -> (points_uv (N,2,P) float32, valid (N,P) bool).  Every cloud is rotated by its viewing angle
    (unless rotate_view is False), moved to (d sin va, cy, d cos va), shifted into the cam0 frame (the reference always
    does; cam0_shift=False projects it where it stands, as the rest of this package does) and projected with cam_p:
    one (3,4) matrix, or (n_cams,3,4) with cam_index (N).  A point is valid where the sum of its rotated |x|, |y|, |z|
    exceeds 0.1; uv is 0 elsewhere."""
    n = int(inst_points_local.shape[0])
    npts = int(np.prod(inst_points_local.shape[1:-1]))
    dev = inst_points_local.device
    x = _placement(xz_dist, centroid_y, viewing_angle, n).to(dev)
    boxes = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    uv, valid, _ = proj_points_err(x, inst_points_local, boxes, cam_p, (1, npts), rotate_view=rotate_view,
                                   cam0_shift=cam0_shift, cam_index=cam_index)
    return uv, valid


# ---------------------------------------------------------------------------------------------- training ground truth

# gen_instance_masks.py: the classes that get an instance id, and each class's inflation of (x, y, z, l, w, h, ry)
REQUIRED_CLASSES = ('Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck', 'Person_sitting', 'Tram', 'Misc')
INFLATIONS = {
    'Car': np.array([1.0, 1.0, 1.0, 1.25, 1.25, 1.1, 1.0]),
    'Van': np.array([1.0, 1.0, 1.0, 1.1, 1.1, 1.05, 1.0]),
    'Truck': np.array([1.0, 1.0, 1.0, 1.1, 1.1, 1.05, 1.0]),
    'Pedestrian': np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.05, 1.0]),
    'Person_sitting': np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.05, 1.0]),
    'Cyclist': np.array([1.0, 1.0, 1.0, 1.1, 1.1, 1.05, 1.0]),
    'Tram': np.array([1.0, 1.0, 1.0, 1.0, 1.1, 1.05, 1.0]),
    'Misc': np.array([1.0, 1.0, 1.0, 1.05, 1.05, 1.05, 1.0]),
}
_INFLATION_OFFSET = np.array([0.0, -0.05, 0.0, 0.0, 0.0, 0.0, 0.0])
BOX_STRIDE = 20  # MPSR_INSTANCE_BOX_STRIDE
MAX_BOXES = 255  # MPSR_INSTANCE_MAX_BOXES


def get_prop_cen_z_offset(class_str):
    """The proposal z centroid offset of a class."""
    offsets = {'Car': 2.17799973487854, 'Pedestrian': 0.351921409368515, 'Cyclist': 0.8944902420043945}
    if class_str not in offsets:
        raise ValueError('Invalid class_str', class_str)
    return offsets[class_str]


def instance_box_table(obj_labels):
    """The per-box constants of one frame for mpsr_instance_images, (n, 20) fp64: the labels of REQUIRED_CLASSES in
    file order (instance id = row of this table), each box_3d (float32) * INFLATIONS[type] + [0, -0.05, 0, ...] in
    fp64, then the u / v / w axes and bounds of points_in_box_3d, computed as the reference orders them, and the
    label's float32 2-D box [y1, x1, y2, x2]."""
    from monopsr_amd.datasets.kitti import obj_utils
    kept = [o for o in obj_labels if o.type in REQUIRED_CLASSES]
    table = np.zeros((len(kept), BOX_STRIDE), np.float64)
    for k, o in enumerate(kept):
        box_3d = obj_utils.object_label_to_box_3d(o) * INFLATIONS[o.type] + _INFLATION_OFFSET
        u, up0, up1, v, vp0, vp3, w, wp0, wp4 = obj_utils.box_3d_slab_bounds(box_3d)
        table[k, 0:15] = np.concatenate([u, [up0, up1], v, [vp0, vp3], w, [wp0, wp4]])
        table[k, 15:19] = obj_utils.object_label_to_box_2d(o)
    return table


def _device(device):
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def _p2_of(calib):
    return np.asarray(getattr(calib, 'p2', calib), np.float64).reshape(3, 4)


def gen_instance_images(depth_maps, calibs, labels_per_frame, device=None):
    """Instance images of F frames of one size: depth_maps (F, H, W) float32 (numpy or CUDA tensor, as read_depth_map
    returns them), calibs F FrameCalibs or (3, 4) P2 matrices, labels_per_frame F lists of ObjectLabels ->
    (F, H, W) uint8 CUDA tensor.  At most 255 labels of REQUIRED_CLASSES per frame."""
    nf = len(labels_per_frame)
    if len(calibs) != nf or len(depth_maps) != nf:
        raise _lib.InvalidArgumentError('gen_instance_images: %d depth maps, %d calibrations, %d label lists'
                                        % (len(depth_maps), len(calibs), nf))
    tables = [instance_box_table(lbl) for lbl in labels_per_frame]
    for f, t in enumerate(tables):
        if len(t) > MAX_BOXES:
            raise _lib.InvalidArgumentError('gen_instance_images: frame %d has %d boxes, at most %d (255 is the '
                                            'background)' % (f, len(t), MAX_BOXES))
    return instance_images_from_tables(depth_maps, [_p2_of(c) for c in calibs], tables, device)


def instance_images_from_tables(depth_maps, p2s, tables, device=None):
    """gen_instance_images on precomputed instance_box_table()s."""
    dev = _device(device)
    with torch.cuda.device(dev):
        depth = torch.as_tensor(depth_maps, device=dev)
        if depth.dim() != 3 or depth.dtype != torch.float32:
            raise _lib.InvalidArgumentError('depth_maps must be (F, H, W) float32, got %s %s'
                                            % (tuple(depth.shape), depth.dtype))
        nf, h, w = depth.shape
        if len(p2s) != nf or len(tables) != nf:
            raise _lib.InvalidArgumentError('instance_images: %d frames, %d P2, %d box tables'
                                            % (nf, len(p2s), len(tables)))
        depth = depth.contiguous()
        offs = np.zeros(nf + 1, np.int64)
        offs[1:] = np.cumsum([len(t) for t in tables])
        tab = np.ascontiguousarray(np.concatenate(list(tables) + [np.zeros((0, BOX_STRIDE))]).astype(np.float64))
        p2 = np.ascontiguousarray(np.stack([np.asarray(p, np.float64).reshape(3, 4) for p in p2s] or
                                           [np.zeros((3, 4))]))
        tab_d = torch.from_numpy(tab).to(dev) if len(tab) else None
        offs_d, p2_d = torch.from_numpy(offs).to(dev), torch.from_numpy(p2).to(dev)
        out = torch.empty((nf, h, w), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().mpsr_instance_images(_lib.ptr(depth), nf, h, w, _lib.ptr(p2_d), _lib.ptr(tab_d),
                                                   _lib.ptr(offs_d), offs.ctypes.data_as(ctypes.c_void_p),
                                                   _lib.ptr(out), _lib.stream()))
    return out


def read_instance_image(instance_image_path):
    """uint8 PNG -> (H, W) uint8 array."""
    from PIL import Image
    return np.asarray(Image.open(instance_image_path), np.uint8)


def save_instance_image(save_path, instance_image):
    from PIL import Image
    img = np.asarray(instance_image)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError('an instance image is (H, W) uint8, got %s %s' % (img.dtype, img.shape))
    Image.fromarray(img).save(save_path, format='PNG')


def get_instance_mask_list(instance_img, num_instances=None):
    """(k, H, W) boolean masks, mask i = (instance_img == i) (the reference's get_instance_mask_list)."""
    if num_instances is None:
        valid_pixels = instance_img[instance_img != 255]
        if len(valid_pixels) == 0:
            return []
        num_instances = np.max(valid_pixels) + 1
    return np.asarray([(instance_img == i) for i in range(num_instances)])


_CENTROID_TYPES = {'bottom': 0, 'middle': 1}


def _crop_args(boxes_2d, frame_index, instance_id, n):
    b2 = np.ascontiguousarray(np.asarray(boxes_2d, np.float32).reshape(-1, 4))
    fi = np.ascontiguousarray(np.asarray(frame_index, np.int32).reshape(-1))
    ii = np.ascontiguousarray(np.asarray(instance_id, np.int32).reshape(-1))
    if not (len(b2) == len(fi) == len(ii) == n):
        raise _lib.InvalidArgumentError('instance_xyz_crops: %d boxes_2d, %d frame indices, %d instance ids, %d boxes_3d'
                                        % (len(b2), len(fi), len(ii), n))
    return b2, fi, ii


def instance_xyz_crops(depth_maps, instance_images, cam_ps, frame_index, instance_id, boxes_2d, boxes_3d, view_angs,
                       roi_size=(48, 48), centroid_type='middle', rotate_view=True, device=None, out=None):
    """The ground truth tf_instance_xyz_crop_from_depth_map builds for every box (monopsr_model.py:158-203) in one
    launch: depth_maps (F, H, W) float32, instance_images (F, H, W) uint8, cam_ps (F, 3, 4); per box frame_index,
    instance_id, boxes_2d [y1, x1, y2, x2] (B, 4), boxes_3d (B, 7), view_angs (B) the estimated (2-D) viewing angles
    -> (xyz_local (B, r, r, 3), xyz_global (B, r, r, 3), valid (B, r, r, 1)) float32 CUDA tensors.  `out`, if given,
    is such a triple to write into.  A box that rounds to an empty crop or one outside the image, a frame or id out of
    range and a non-square roi_size raise InvalidArgumentError."""
    dev = _device(device)
    roi_h, roi_w = (int(roi_size), int(roi_size)) if np.ndim(roi_size) == 0 else (int(roi_size[0]), int(roi_size[1]))
    if centroid_type not in _CENTROID_TYPES:
        raise _lib.InvalidArgumentError('centroid_type must be bottom or middle, got %r' % (centroid_type,))
    with torch.cuda.device(dev):
        f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32) if not torch.is_tensor(a) else a, device=dev) \
            .float().contiguous()
        depth = f32(depth_maps)
        if not torch.is_tensor(instance_images):
            instance_images = np.require(instance_images, requirements=['C', 'W'])  # (PNG arrays are read-only)
        inst = torch.as_tensor(instance_images, device=dev).contiguous()
        if depth.dim() != 3 or tuple(inst.shape) != tuple(depth.shape) or inst.dtype != torch.uint8:
            raise _lib.InvalidArgumentError('depth_maps (F, H, W) float32 and instance_images (F, H, W) uint8, got %s '
                                            'and %s %s' % (tuple(depth.shape), tuple(inst.shape), inst.dtype))
        nf, h, w = depth.shape
        p2 = f32(cam_ps).reshape(-1)
        if p2.numel() != 12 * nf:
            raise _lib.InvalidArgumentError('cam_ps must be (F, 3, 4)')
        b3 = f32(boxes_3d).reshape(-1, 7)
        n = b3.shape[0]
        host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
        b2_h, fi_h, ii_h = _crop_args(host(boxes_2d), host(frame_index), host(instance_id), n)
        va = f32(view_angs).reshape(-1)
        if va.numel() != n:
            raise _lib.InvalidArgumentError('view_angs must hold one angle per box')
        b2, fi, ii = (torch.from_numpy(a).to(dev) for a in (b2_h, fi_h, ii_h))
        if out is None:
            out = (torch.empty((n, roi_h, roi_w, 3), dtype=torch.float32, device=dev),
                   torch.empty((n, roi_h, roi_w, 3), dtype=torch.float32, device=dev),
                   torch.empty((n, roi_h, roi_w, 1), dtype=torch.float32, device=dev))
        loc, glob, valid = out
        for t, c in ((loc, 3), (glob, 3), (valid, 1)):
            if tuple(t.shape) != (n, roi_h, roi_w, c) or t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.InvalidArgumentError('out tensors must be contiguous float32 (B, r, r, 3/3/1)')
        _lib.check(_lib.lib().mpsr_instance_xyz_crops(
            _lib.ptr(depth), _lib.ptr(inst), _lib.ptr(p2), nf, h, w, _lib.ptr(fi), _lib.ptr(ii), _lib.ptr(b2),
            _lib.ptr(b3), _lib.ptr(va), fi_h.ctypes.data_as(ctypes.c_void_p), ii_h.ctypes.data_as(ctypes.c_void_p),
            b2_h.ctypes.data_as(ctypes.c_void_p), n, roi_h, roi_w, _CENTROID_TYPES[centroid_type], int(bool(rotate_view)),
            _lib.ptr(loc), _lib.ptr(glob), _lib.ptr(valid), _lib.stream()))
    return loc, glob, valid


def save_instance_images(split_dir, depth_dir, out_dir, frames=None, batch=8, log=None):
    """gen_instance_masks.py for split_dir (label_2/, calib/, optionally image_2/) and depth_dir/<name>.png into
    out_dir/<name>.png.  Returns the names written, in the order written."""
    from monopsr_amd.datasets.kitti import depth_map_utils, obj_utils
    if batch < 1:
        raise ValueError('batch must be >= 1, got %d' % batch)
    if frames is None:
        if not os.path.isdir(depth_dir):
            raise FileNotFoundError('no such depth directory: %s' % depth_dir)
        frames = sorted(f[:-4] for f in os.listdir(depth_dir) if f.endswith('.png'))
    shapes = {}
    for n in frames:
        shapes[n] = depth_map_utils.image_shape(os.path.join(depth_dir, n + '.png'))
        img = os.path.join(split_dir, 'image_2', n + '.png')
        if os.path.exists(img) and depth_map_utils.image_shape(img) != shapes[n]:
            raise ValueError('frame %s: image_2 is %s but its depth map is %s'
                             % (n, depth_map_utils.image_shape(img), shapes[n]))
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for _, names in depth_map_utils._groups(frames, shapes, batch):
        depths = np.stack([depth_map_utils.read_depth_map(os.path.join(depth_dir, n + '.png')) for n in names])
        calibs = [depth_map_utils.read_calibration(os.path.join(split_dir, 'calib', n + '.txt')) for n in names]
        labels = [obj_utils.read_labels(os.path.join(split_dir, 'label_2'), n) for n in names]
        images = gen_instance_images(depths, calibs, labels).cpu().numpy()
        for n, im in zip(names, images):
            save_instance_image(os.path.join(out_dir, n + '.png'), im)
            written.append(n)
        if log:
            log('%d / %d frames' % (len(written), len(frames)))
    return written


def main(argv=None):
    p = argparse.ArgumentParser(prog='python -m monopsr_amd.datasets.kitti.instance_utils',
                                description='KITTI instance images (255 = background, k = k-th label) on the GPU.')
    p.add_argument('split_dir', help='KITTI split directory with label_2/ and calib/ (image_2/ is checked if present)')
    p.add_argument('depth_dir', help='directory of <name>.png depth maps (depth_map_utils writes them)')
    p.add_argument('out_dir', help='directory for <name>.png')
    p.add_argument('--frames', nargs='+', help='frame names (default: every depth map in depth_dir)')
    p.add_argument('--batch', type=int, default=8, help='frames per launch (default 8)')
    a = p.parse_args(argv)
    if a.batch < 1:
        p.error('--batch must be >= 1')
    for d in (a.split_dir, a.depth_dir):
        if not os.path.isdir(d):
            p.error('no such directory: %s' % d)
    names = save_instance_images(a.split_dir, a.depth_dir, a.out_dir, a.frames, a.batch,
                                 log=lambda m: print(m, file=sys.stderr))
    print('wrote %d instance images to %s' % (len(names), a.out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
