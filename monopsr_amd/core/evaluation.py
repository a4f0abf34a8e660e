"""Box and mask overlaps on device tensors: the names of the reference's core/evaluation.py (mask_iou, two_d_iou,
three_d_iou) with bev_iou and paired_overlaps next to them.  DESIGN.md section 7.11.

    iou = three_d_iou(box, boxes)          # box (7,), boxes (N, 7) [ry, l, h, w, tx, ty, tz] -> (N,) float64
    iou = two_d_iou(box, boxes)            # box (4,), boxes (N, 4) [x1, y1, x2, y2]          -> (N,) float64
    table, overlaps, bins = paired_overlaps(pred_box_3d, gt_box_3d, fed_box_2d, label_info)   # row k against row k

One box against many is one mpsr_kitti_overlaps launch over a frame of one detection and N ground truths: the boxes
are widened to float64 without loss, whatever their dtype.  paired_overlaps is mpsr_object_pairs, whose inputs are
float32.  Both run the one body of csrc/kitti_geometry.h: exact clipping of the two bases in fp64.

Where the reference differs: its three_d_iou rasterises both bases at 1 cm with PIL (outlines included) and caps the
base intersection at 100 m^2; here the intersection is exact and uncapped (on the reference's own 174 recorded pins the
two differ by at most 0.0168).  It returns a scalar for a single box; here the result is always (N,).  Its sphere
pre-test changes no value.  evaluate_2d, evaluate_3d and the average-recall helpers, which nothing in the reference
calls, are not built.
"""
import ctypes

import numpy as np
import torch

from monopsr_amd import _lib
from monopsr_amd.core import evaluator_utils, kitti_eval


def _one_against_many(det_row, gt_rows):
    """mpsr_kitti_overlaps' six overlaps of one detection row (FIELDS,) against gt_rows (N, FIELDS), float64 on the
    device -> (6, N) float64 on the device."""
    dev = gt_rows.device
    n = int(gt_rows.shape[0])
    with torch.cuda.device(dev):
        out = torch.empty((6, n), dtype=torch.float64, device=dev)
        if n == 0:
            return out
        det = det_row.reshape(1, kitti_eval.FIELDS).contiguous()
        gt = gt_rows.contiguous()
        dof, gof, pof = np.array([0, 1], np.int32), np.array([0, n], np.int32), np.array([0, n], np.int64)
        ints = torch.zeros(n + 1, dtype=torch.int32, device=dev)  # the class codes: not read by the overlaps
        dof_d, gof_d, pof_d = (torch.from_numpy(a).to(dev) for a in (dof, gof, pof))
        p = _lib.ptr
        batch = _lib.KittiBatch(p(det), p(ints[0:1]), p(gt), p(ints[1:]), p(dof_d), p(gof_d), p(pof_d),
                                dof.ctypes.data, gof.ctypes.data, pof.ctypes.data, 1, n, 1)
        _lib.check(_lib.lib().mpsr_kitti_overlaps(ctypes.byref(batch), p(out), _lib.stream()))
    return out


def _rows(boxes, width, columns, what):
    """boxes (N, width) -> (N, FIELDS) float64 rows with `columns` filled, zero elsewhere."""
    _lib.ptr(boxes[0:0])  # (refuses tensors that are not on the GPU)
    if boxes.dim() != 2 or int(boxes.shape[1]) != width:
        raise ValueError('%s: boxes must be (N, %d), got %s' % (what, width, tuple(boxes.shape)))
    rows = torch.zeros((int(boxes.shape[0]), kitti_eval.FIELDS), dtype=torch.float64, device=boxes.device)
    rows[:, columns] = boxes.double()
    return rows


def _box_and_boxes(box, boxes, width, columns, what):
    if boxes.dim() == 1:
        boxes = boxes[None]
    if box.numel() != width:
        raise ValueError('%s: box must hold %d values, got %s' % (what, width, tuple(box.shape)))
    return _rows(box.reshape(1, width).to(boxes.device), width, columns, what)[0], _rows(boxes, width, columns, what)


_IMAGE_COLUMNS = [kitti_eval.X1, kitti_eval.Y1, kitti_eval.X2, kitti_eval.Y2]
_BOX_COLUMNS = [kitti_eval.RY, kitti_eval.L, kitti_eval.H, kitti_eval.W, kitti_eval.TX, kitti_eval.TY, kitti_eval.TZ]


def two_d_iou(box, boxes):
    """The IoU of box (4,) [x1, y1, x2, y2] with every row of boxes (N, 4): (N,) float64 on the device."""
    return _one_against_many(*_box_and_boxes(box, boxes, 4, _IMAGE_COLUMNS, 'two_d_iou'))[0]


def three_d_iou(box, boxes):
    """The 3-D IoU of box (7,) [ry, l, h, w, tx, ty, tz] (ty on the bottom face) with every row of boxes (N, 7):
    (N,) float64 on the device.  Non-positive l, w or h on either box gives 0."""
    return _one_against_many(*_box_and_boxes(box, boxes, 7, _BOX_COLUMNS, 'three_d_iou'))[2]


def bev_iou(box, boxes):
    """The IoU of the bases (bird's-eye view) of three_d_iou's boxes: (N,) float64 on the device."""
    return _one_against_many(*_box_and_boxes(box, boxes, 7, _BOX_COLUMNS, 'bev_iou'))[1]


def paired_overlaps(pred_box_3d, gt_box_3d, fed_box_2d=None, label_info=None,
                    depth_edges=evaluator_utils.DEFAULT_DEPTH_EDGES,
                    box_iou_edges=evaluator_utils.DEFAULT_BOX_IOU_EDGES):
    """Row k of pred_box_3d against row k of gt_box_3d, (n, 7) [x y z l w h ry] float32: evaluator_utils.object_pairs
    -> (table (n, 9) float32, overlaps (n, 4) float64 [iou_2d_fed, iou_bev, iou_3d, centre_dist], bins (n, 3) int32)."""
    return evaluator_utils.object_pairs(pred_box_3d, gt_box_3d, fed_box_2d, label_info, depth_edges, box_iou_edges)


def mask_iou(mask1, mask2):
    """The IoU of two masks of one shape (non-zero = set), device tensors: a float64 scalar on the device, NaN when
    both are empty (the reference divides 0 by 0)."""
    _lib.ptr(mask1.reshape(-1)[0:0]), _lib.ptr(mask2.reshape(-1)[0:0])
    if mask1.shape != mask2.shape:
        raise ValueError('mask_iou: shapes %s and %s' % (tuple(mask1.shape), tuple(mask2.shape)))
    a, b = mask1 != 0, mask2 != 0
    return (a & b).sum().double() / (a | b).sum().double()
