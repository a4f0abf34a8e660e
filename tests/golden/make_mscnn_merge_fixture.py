"""Records tests/golden/mscnn_merge.npz: the outputs of the reference's own merge_kitti_and_mscnn_obj_labels on the
catalogue of tests/merge_cases.py.  Needs the reference tree: python make_mscnn_merge_fixture.py <reference>/src.
The fixture holds, per case, the catalogue's boxes and scores and the reference's merged boxes and scores only."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merge_cases  # noqa: E402


def _import_reference(src):
    sys.path.insert(0, src)
    try:
        import cv2  # noqa: F401
    except ImportError:
        import cv2_standin
        sys.modules['cv2'] = cv2_standin
    # modules the reference imports at load time and the merge never calls: an empty stand-in for each missing one
    for _ in range(64):
        try:
            from monopsr.datasets.kitti import obj_utils
            return obj_utils
        except ModuleNotFoundError as e:
            if e.name.split('.')[0] == 'monopsr':
                raise
            mod = types.ModuleType(e.name)
            mod.__path__ = []
            sys.modules[e.name] = mod
            if '.' in e.name:
                parent, _, leaf = e.name.rpartition('.')
                setattr(sys.modules[parent], leaf, mod)
            for key in [k for k in sys.modules if k.startswith('monopsr')]:
                del sys.modules[key]
    from monopsr.datasets.kitti import obj_utils
    return obj_utils


def main(src):
    obj_utils = _import_reference(src)
    out = {}

    def labels(boxes, z, scores=None):
        objs = []
        for k, b in enumerate(boxes):
            o = obj_utils.ObjectLabel()
            o.type = 'Car'
            o.y1, o.x1, o.y2, o.x2 = b
            o.t = np.asarray([0.0, 1.5, z[k] if z is not None else 10.0], np.float32)
            o.score = float(scores[k]) if scores is not None else 0.0
            objs.append(o)
        return objs

    for c in merge_cases.catalogue():
        name = c['name']
        for key in ('label_boxes', 'label_z', 'det_boxes', 'det_scores'):
            out['%s/%s' % (name, key)] = c[key]
        out['%s/min_iou' % name] = np.float64(c['min_iou'])
        out['%s/score_type' % name] = np.array(c['score_type'])
        if not len(c['label_boxes']):
            continue  # the reference's np.argmax raises on a frame without labels (or returns nothing to record)
        merged = obj_utils.merge_kitti_and_mscnn_obj_labels(
            labels(c['label_boxes'], c['label_z']), labels(c['det_boxes'], None, c['det_scores']), c['min_iou'],
            c['score_type'])
        out['%s/ref_boxes' % name] = np.asarray([[o.y1, o.x1, o.y2, o.x2] for o in merged], np.float64).reshape(-1, 4)
        out['%s/ref_scores' % name] = np.asarray([o.score for o in merged], np.float64)
    np.savez_compressed(os.path.join(HERE, 'mscnn_merge.npz'), **out)
    print('recorded %d arrays' % len(out))


if __name__ == '__main__':
    main(sys.argv[1])
