"""A restatement in numpy of what mpsr_merge_detections computes (monopsr_amd/csrc/detections.hip): the reference's
obj_utils.merge_kitti_and_mscnn_obj_labels (obj_utils.py:1037-1089) on arrays, written from its description.

Dtypes, as the reference forms them: boxes_2d_from_obj_labels gives float32 boxes; two_d_iou of
datasets/kitti/evaluation.py (:6-44, the module obj_utils imports; core/evaluation.py holds a twin that does not round)
multiplies, adds and divides them in float32, stores the quotient into a float64 array and returns iou.round(3), which
is rint(x * 1000) / 1000 in fp64.  np.argmax and `matching_iou >= min_iou` see the rounded fp64 values.  The fallback score is taken in float32 here (np.float32 / 45.0 stays float32
under NumPy >= 2; NumPy 1.x widened a scalar pair to fp64, and the sample's label_scores is float32 either way).
"""
import numpy as np

SCORE_TYPES = {'distance': 0, 'max': 1, 'min': 2}
f32 = np.float32


def two_d_iou(box, boxes):
    """two_d_iou (datasets/kitti/evaluation.py:6-44) of float32 [y1, x1, y2, x2] boxes -> float64 (n,)."""
    box, boxes = np.asarray(box, f32), np.asarray(boxes, f32).reshape(-1, 4)
    iou = np.zeros(len(boxes), np.float64)
    x1_int, y1_int = np.maximum(box[0], boxes[:, 0]), np.maximum(box[1], boxes[:, 1])
    x2_int, y2_int = np.minimum(box[2], boxes[:, 2]), np.minimum(box[3], boxes[:, 3])
    w_int, h_int = (x2_int - x1_int).astype(f32), (y2_int - y1_int).astype(f32)
    non_empty = (w_int > 0) & (h_int > 0)
    if non_empty.any():
        inter = (w_int[non_empty] * h_int[non_empty]).astype(f32)
        box_area = f32(f32(box[2] - box[0]) * f32(box[3] - box[1]))
        boxes_area = ((boxes[non_empty, 2] - boxes[non_empty, 0]).astype(f32) *
                      (boxes[non_empty, 3] - boxes[non_empty, 1]).astype(f32)).astype(f32)
        union = ((box_area + boxes_area).astype(f32) - inter).astype(f32)
        iou[non_empty] = (inter / union).astype(f32)
    return np.rint(iou * 1000.0) / 1000.0


def merge_frame(label_boxes, label_z, det_boxes, det_scores, min_iou, score_type='distance'):
    """One frame.  label_boxes (L,4), det_boxes (D,4) [y1, x1, y2, x2]; label_z (L,); det_scores (D,) fp64.
    -> (boxes (L,4) float32, scores (L,) float64, match (L,) int32: the detection that wrote the label, or -1).
    A frame without labels merges nothing (the reference's np.argmax raises there)."""
    kitti = np.asarray(label_boxes, f32).reshape(-1, 4)
    dets = np.asarray(det_boxes, f32).reshape(-1, 4)
    det_scores = np.asarray(det_scores, np.float64).reshape(-1)
    z = np.asarray(label_z, f32).reshape(-1)
    boxes, scores, match = kitti.copy(), np.zeros(len(kitti), np.float64), np.full(len(kitti), -1, np.int32)
    if len(kitti):
        for d in range(len(dets)):
            iou = two_d_iou(dets[d], kitti)  # always against the original boxes
            k = int(np.argmax(iou))
            if iou[k] >= min_iou:
                boxes[k], scores[k], match[k] = dets[d], det_scores[d], d
    code = SCORE_TYPES[score_type]
    for k in range(len(kitti)):
        if scores[k] == 0:
            if code == 0:
                s = f32(f32(1.0) - f32(z[k] / f32(45.0)))
                scores[k] = np.float64(min(max(s, f32(0.1)), f32(1.0)))
            elif code == 1:
                scores[k] = 1.0
    return boxes, scores, match
