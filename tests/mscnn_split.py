"""The five-frame fixture split of tests/test_kitti_dataset_gpu.py, one more frame, and synthetic MSCNN detection files, shared by
tests/test_kitti_dataset_mscnn_gpu.py and tests/test_evaluator_gpu.py."""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
# name in the split -> fixture frame; 000010 is frame 000006 again.  000000 holds one Pedestrian and keeps no label.
SPLIT = (('000000', '000000'), ('000006', '000006'), ('000001', '000001'), ('000010', '000006'), ('000002', '000002'),
         ('000011', '000001'))
NAMES = [n for n, _ in SPLIT]
# box_2d_height 20: the Car of 000001 is 21.58 px high; its detection (IoU 0.90) is 19.5 px high
# 000011 is frame 000001 with its Car lowered to 19.0 px: under box_2d_height on KITTI's box, while its detection
# (IoU 0.88) is 21.5 px high.  The merged labels keep it, the original labels keep nothing: the reference's second check.
LABEL_EDITS = {'000011': ('387.63 181.54 423.81 203.12', '387.63 181.54 423.81 200.54')}
FILTER = dict(difficulty_str='all', box_2d_height=20, truncation=None, occlusion=None, depth_range=[5, 80])


def _det(cls, x1, y1, x2, y2, score):
    return '%s -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10 %.4f' % (cls, x1, y1, x2, y2, score)


DETECTIONS = {
    '000000': [_det('Pedestrian', 713.0, 144.0, 811.0, 306.0, 0.91)],
    # the four cars shifted by a pixel or two (the second one twice: the later file row wins), one far-off false positive
    '000006': [_det('Car', 549.0, 172.0, 573.0, 195.0, 0.55), _det('Car', 506.0, 169.0, 577.0, 210.0, 0.97),
               _det('Car', 900.0, 50.0, 960.0, 90.0, 0.31), _det('Car', 51.0, 184.5, 226.0, 248.0, 0.88),
               _det('Car', 504.5, 168.0, 575.0, 208.5, 0.93), _det('Car', 329.5, 171.5, 398.0, 203.0, 0.76)],
    '000001': [_det('Car', 387.63, 182.5, 423.81, 202.0, 0.62)],
    # two of the four cars only: the others take the distance score
    '000010': [_det('Car', 506.0, 169.0, 577.0, 210.0, 0.97), _det('Car', 51.0, 184.5, 226.0, 248.0, 0.88)],
    '000002': [],
    '000011': [_det('Car', 387.63, 181.0, 423.81, 202.5, 0.71)],
}


def build(top, with_labels=True):
    """dataset_dir `top` with train.txt / val.txt, training/{calib, image_2[, label_2, depth_2_multiscale,
    instance_2_depth_2_multiscale]} and mscnn/<name>.txt.  -> (dataset_dir, mscnn_label_dir)."""
    fix = np.load(os.path.join(GOLDEN, 'instance_fixture.npz'))
    split = os.path.join(top, 'training')
    dirs = ['calib', 'image_2'] + (['label_2', 'depth_2_multiscale', 'instance_2_depth_2_multiscale']
                                   if with_labels else [])
    for d in dirs:
        os.makedirs(os.path.join(split, d))
    mscnn = os.path.join(top, 'mscnn')
    os.makedirs(mscnn)
    rng = np.random.default_rng(0)
    for name, f in SPLIT:
        depth = Image.open(os.path.join(GOLDEN, 'depth_%s.png' % f))
        p2 = ' '.join('%.12e' % v for v in fix['p2_%s' % f].reshape(-1))
        with open(os.path.join(split, 'calib', name + '.txt'), 'w') as out:
            out.write('P2: %s\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\n' % p2)
        w, h = depth.size
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(
            os.path.join(split, 'image_2', name + '.png'))
        if with_labels:
            with open(os.path.join(split, 'label_2', name + '.txt'), 'w') as out:
                text = str(fix['labels_%s' % f])
                if name in LABEL_EDITS:
                    assert LABEL_EDITS[name][0] in text
                    text = text.replace(*LABEL_EDITS[name])
                out.write(text)
            depth.save(os.path.join(split, 'depth_2_multiscale', name + '.png'))
            Image.open(os.path.join(GOLDEN, 'instance_%s.png' % f)).save(
                os.path.join(split, 'instance_2_depth_2_multiscale', name + '.png'))
        with open(os.path.join(mscnn, name + '.txt'), 'w') as out:
            out.write(''.join(line + '\n' for line in DETECTIONS[name]))
    for s in ('train', 'val'):
        with open(os.path.join(top, s + '.txt'), 'w') as out:
            out.write(''.join(name + '\n' for name in NAMES))
    return top, mscnn


def config(root, data_split='val', num_boxes=8, **over):
    from monopsr_amd.core.config_utils import ConfigObj
    cfg = dict(name='kitti', dataset_dir=root, data_split=data_split, data_split_dir='training', num_boxes=num_boxes,
               classes=['Car'], oversample=True, num_alpha_bins=12, alpha_bin_overlap=0.0, use_mscnn_detections=True,
               obj_filter_config=dict(FILTER), aug_config=dict(use_image_aug=False, box_jitter_type='oversample'),
               depth_version='multiscale', instance_version='depth_2_multiscale')
    cfg.update(over)
    return ConfigObj(cfg)
