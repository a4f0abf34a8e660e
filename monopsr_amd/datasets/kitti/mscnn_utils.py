"""Merging MSCNN 2-D detections into KITTI labels on the GPU: obj_utils.merge_kitti_and_mscnn_obj_labels of the
reference (obj_utils.py:1037-1089) for all frames of a split in one mpsr_merge_detections launch.

    boxes, scores, match = merge_frames(label_boxes, label_z, det_boxes, det_scores, min_iou=0.7)
    merged = merged_obj_labels(kitti_obj_labels_of_frame_k, boxes[k], scores[k])
"""
import copy

import numpy as np
import torch

from monopsr_amd import _lib

SCORE_TYPES = {'distance': 0, 'max': 1, 'min': 2}  # MPSR_MERGE_SCORE_*
MIN_IOU = {'Car': 0.7, 'Pedestrian': 0.5, 'Cyclist': 0.5}  # kitti_dataset.py:78-81


def merge_frames(label_boxes, label_z, det_boxes, det_scores, min_iou, default_score_type='distance', device=None):
    """Per-frame lists: label_boxes[f] (L_f, 4) and det_boxes[f] (D_f, 4) [y1, x1, y2, x2], label_z[f] (L_f,) the
    labels' t[2], det_scores[f] (D_f,).  One upload, one launch, one copy back.
    -> per-frame lists (boxes (L_f, 4) float32, scores (L_f,) float64, match (L_f,) int32: the index of the detection
    that wrote the label, or -1)."""
    if default_score_type not in SCORE_TYPES:
        raise ValueError('Invalid default score type', default_score_type)
    nf = len(label_boxes)
    if not (len(label_z) == len(det_boxes) == len(det_scores) == nf):
        raise ValueError('merge_frames: the four lists must hold one entry per frame')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    lb = [np.asarray(b, np.float32).reshape(-1, 4) for b in label_boxes]
    db = [np.asarray(b, np.float32).reshape(-1, 4) for b in det_boxes]
    lz = [np.asarray(z, np.float32).reshape(-1) for z in label_z]
    ds = [np.asarray(s, np.float64).reshape(-1) for s in det_scores]
    for f in range(nf):
        if len(lz[f]) != len(lb[f]) or len(ds[f]) != len(db[f]):
            raise ValueError('merge_frames: frame %d has %d boxes for %d z, %d detections for %d scores'
                             % (f, len(lb[f]), len(lz[f]), len(db[f]), len(ds[f])))
    loff = np.concatenate([[0], np.cumsum([len(b) for b in lb])]).astype(np.int64)
    doff = np.concatenate([[0], np.cumsum([len(b) for b in db])]).astype(np.int64)
    nl, nd = int(loff[-1]), int(doff[-1])
    up = lambda parts, dt, shape: torch.from_numpy(np.ascontiguousarray(
        np.concatenate(parts + [np.zeros(shape, dt)]))).to(dev)
    with torch.cuda.device(dev):
        lb_d, lz_d = up(lb, np.float32, (0, 4)), up(lz, np.float32, (0,))
        db_d, ds_d = up(db, np.float32, (0, 4)), up(ds, np.float64, (0,))
        loff_d, doff_d = torch.from_numpy(loff).to(dev), torch.from_numpy(doff).to(dev)
        # one buffer for the three outputs: 4 float32 + 1 float64 + 1 int32 per label, copied back at once
        out = torch.zeros(max(nl, 1) * 28, dtype=torch.uint8, device=dev)
        scores_d = out[0:8 * nl].view(torch.float64)
        boxes_d = out[8 * nl:24 * nl].view(torch.float32)
        match_d = out[24 * nl:28 * nl].view(torch.int32)
        _lib.check(_lib.lib().mpsr_merge_detections(
            _lib.ptr(lb_d), _lib.ptr(lz_d), _lib.ptr(loff_d), nl, _lib.ptr(db_d), _lib.ptr(ds_d), _lib.ptr(doff_d), nd,
            nf, float(min_iou), SCORE_TYPES[default_score_type], _lib.ptr(boxes_d), _lib.ptr(scores_d),
            _lib.ptr(match_d), _lib.stream()))
        host = out.cpu().numpy()
    scores = host[0:8 * nl].view(np.float64)
    boxes = host[8 * nl:24 * nl].view(np.float32).reshape(-1, 4)
    match = host[24 * nl:28 * nl].view(np.int32)
    cut = lambda a: [a[loff[f]:loff[f + 1]].copy() for f in range(nf)]
    return cut(boxes), cut(scores), cut(match)


def label_arrays(obj_labels):
    """(boxes (n, 4) float32 [y1, x1, y2, x2], z (n,) float32, scores (n,) float64) of parsed labels."""
    n = len(obj_labels)
    boxes = np.asarray([[o.y1, o.x1, o.y2, o.x2] for o in obj_labels], np.float32).reshape(n, 4)
    z = np.asarray([o.t[2] for o in obj_labels], np.float32).reshape(n)
    return boxes, z, np.asarray([o.score for o in obj_labels], np.float64).reshape(n)


def merged_obj_labels(kitti_obj_labels, boxes, scores):
    """Copies of the KITTI labels with the merged boxes and scores (the reference's new_kitti_labels)."""
    out = copy.deepcopy(kitti_obj_labels)
    for o, b, s in zip(out, boxes, scores):
        o.y1, o.x1, o.y2, o.x2 = np.float32(b[0]), np.float32(b[1]), np.float32(b[2]), np.float32(b[3])
        o.score = float(s)
    return out
