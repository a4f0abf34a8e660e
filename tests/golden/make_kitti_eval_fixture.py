"""Generates tests/golden/kitti_eval.npz -- label files and overlap pins for the KITTI evaluation tests.

Run in the build container only (reads the reference's own test fixture, the mini KITTI tree under
/root/reference/src/monopsr/tests/datasets/Kitti/object, and its Python geometry; the GPU box never has them):

    python tests/golden/make_kitti_eval_fixture.py

What is stored (numpy + PIL only):
  * the 13 training/label_2 files of the mini tree, verbatim (`label_names`, `label_texts`): 35 Car, 14 Pedestrian,
    6 Cyclist, 1 Van, 26 DontCare (and one Truck, one Misc);
  * 2-D pins: the REFERENCE's monopsr.core.evaluation.two_d_iou between each non-DontCare label box [x1,y1,x2,y2] and
    three seeded perturbations of it, and between the boxes of each frame (`pin2d_a`, `pin2d_b`, `pin2d_iou`);
  * 3-D pins: the reference's three_d_iou (a 1 cm raster of the two bases, evaluation.py:203-282) between each
    non-DontCare label box and three seeded perturbations of it (`pin3d_a`, `pin3d_b`, `pin3d_iou`).  The rows are
    [ry, l, h, w, tx, ty, tz] built from the label fields directly (box_3d_to_3d_iou_format puts w where h belongs).
The file holds data only.
"""
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference/src")
from monopsr.core import evaluation  # noqa: E402

LABELS = "/root/reference/src/monopsr/tests/datasets/Kitti/object/training/label_2"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    names = sorted(os.listdir(LABELS))
    texts = [open(os.path.join(LABELS, n), newline="").read() for n in names]
    rng = np.random.default_rng(0)
    a2, b2, a3, b3 = [], [], [], []
    for text in texts:
        boxes2, boxes3 = [], []
        for line in text.splitlines():
            t = line.split()
            if not t or t[0] == "DontCare":
                continue
            v = [float(x) for x in t[1:]]
            x1, y1, x2, y2 = v[3:7]
            h, w, l, tx, ty, tz, ry = v[7:14]
            boxes2.append([x1, y1, x2, y2])
            boxes3.append([ry, l, h, w, tx, ty, tz])
        for bx in boxes2:
            for _ in range(3):
                wd, ht = bx[2] - bx[0], bx[3] - bx[1]
                c = rng.normal(0, 0.15, 2) * [wd, ht]
                s = rng.uniform(0.7, 1.3, 2)
                cx, cy = (bx[0] + bx[2]) / 2 + c[0], (bx[1] + bx[3]) / 2 + c[1]
                a2.append(bx)
                b2.append([cx - wd * s[0] / 2, cy - ht * s[1] / 2, cx + wd * s[0] / 2, cy + ht * s[1] / 2])
        for i in range(len(boxes2)):
            for j in range(len(boxes2)):
                if i != j:
                    a2.append(boxes2[i])
                    b2.append(boxes2[j])
        for bx in boxes3:
            for _ in range(3):
                p = list(bx)
                p[0] += rng.normal(0, 0.3)
                p[1] *= rng.uniform(0.8, 1.2)
                p[2] *= rng.uniform(0.8, 1.2)
                p[3] *= rng.uniform(0.8, 1.2)
                p[4] += rng.normal(0, 0.25 * bx[1])
                p[5] += rng.normal(0, 0.2 * bx[2])
                p[6] += rng.normal(0, 0.25 * bx[1])
                a3.append(bx)
                b3.append(p)
    a2, b2, a3, b3 = [np.array(x, np.float64) for x in (a2, b2, a3, b3)]
    iou2 = np.array([evaluation.two_d_iou(a, b[None])[0] for a, b in zip(a2, b2)], np.float64)
    iou3 = np.array([float(evaluation.three_d_iou(a, b[None])) for a, b in zip(a3, b3)], np.float64)
    np.savez_compressed(os.path.join(HERE, "kitti_eval.npz"), label_names=np.array(names),
                        label_texts=np.array(texts), pin2d_a=a2, pin2d_b=b2, pin2d_iou=iou2, pin3d_a=a3, pin3d_b=b3,
                        pin3d_iou=iou3)
    print("wrote %d label files, %d 2-D pins, %d 3-D pins (%d with overlap)"
          % (len(names), len(iou2), len(iou3), int((iou3 > 0).sum())))


if __name__ == "__main__":
    main()
