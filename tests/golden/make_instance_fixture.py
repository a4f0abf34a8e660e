"""Generates the instance fixtures: tests/golden/instance_<frame>.png and instance_fixture.npz.

Run in the build container only (reads the reference's mini KITTI tree and imports its code; the GPU box has neither):

    python tests/golden/make_instance_fixture.py

It runs the reference's UNMODIFIED demos/instances/gen_instance_masks.main() on frames 000000, 000001, 000002 and 000006
with the committed depth maps tests/golden/depth_<frame>.png as its depth directory, through a stub DatasetBuilder, with
tests/cv2_standin.py (given imread / imwrite here) installed as `cv2` and empty modules as `tensorflow` and `png`.

numpy >= 2 promotes `depth_map / cam_p[0, 0]` (float32 array / float64 scalar) to float64, which numpy 1 -- what the
reference was written for -- kept in float32.  The frame calibrations handed to the reference hold a P2 whose scalar
elements come back as Python floats, which numpy 2 treats as numpy 1 treated a float64 scalar: the numpy 1 meaning.
The fixture records that as `division = 'numpy1'`.

Before writing anything it ASSERTS that tests/instance_restatement.py equals the reference's images bit for bit, and the
project's label, filter, viewing-angle, mean-lwh and prop-offset helpers equal the reference's.  Then it writes data only:
the four instance images as PNGs, each frame's label text and P2, and the reference's host-side values.
"""
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
import cv2_standin  # noqa: E402
import instance_restatement as rs  # noqa: E402
from monopsr_amd.datasets.kitti import obj_utils as my_obj  # noqa: E402
from monopsr_amd.datasets.kitti import instance_utils as my_iu  # noqa: E402


def _imread(path, flags=None):
    if flags == cv2_standin.IMREAD_ANYDEPTH:
        return np.asarray(Image.open(path))
    return np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))[..., ::-1])


WRITTEN = {}


def _imwrite(path, img, *a):
    WRITTEN[os.path.basename(path)[:-4]] = np.array(img)
    return True


cv2_standin.IMREAD_ANYDEPTH = 2
cv2_standin.imread = _imread
cv2_standin.imwrite = _imwrite
cv2_standin.IMWRITE_PNG_COMPRESSION = 16
sys.modules['cv2'] = cv2_standin
sys.modules['tensorflow'] = types.ModuleType('tensorflow')
sys.modules['png'] = types.ModuleType('png')
if not hasattr(np, 'bool'):
    np.bool = bool
sys.path.insert(0, '/root/reference/src')
sys.path.insert(0, '/root/reference/demos/instances')

KITTI = '/root/reference/src/monopsr/tests/datasets/Kitti/object/training'
FRAMES = ('000000', '000001', '000002', '000006')


class _ScalarFloats(np.ndarray):
    """A P2 whose scalar elements are Python floats (numpy 1's value-based casting of `f32_array / cam_p[0, 0]`)."""

    def __getitem__(self, key):
        v = super().__getitem__(key)
        return float(v) if np.ndim(v) == 0 else v


class _Dataset:
    def __init__(self, depth_dir):
        self.image_2_dir = os.path.join(KITTI, 'image_2')
        self.calib_dir = os.path.join(KITTI, 'calib')
        self.kitti_label_dir = os.path.join(KITTI, 'label_2')
        self.depth_dir = depth_dir
        self.num_samples = len(FRAMES)

    @staticmethod
    def get_sample_names():
        return list(FRAMES)


def _install_stubs(depth_dir):
    builders = types.ModuleType('monopsr.builders.dataset_builder')

    class DatasetBuilder:
        KITTI_TRAINVAL = 'trainval'

        @staticmethod
        def build_kitti_dataset(_cfg):
            return _Dataset(depth_dir)

    builders.DatasetBuilder = DatasetBuilder
    sys.modules['monopsr.builders.dataset_builder'] = builders
    from monopsr.datasets.kitti import calib_utils
    read = calib_utils.read_frame_calib

    def read_frame_calib(path):
        calib = read(path)
        calib.p2 = np.asarray(calib.p2, np.float64).view(_ScalarFloats)
        return calib

    calib_utils.read_frame_calib = read_frame_calib


def main():
    tmp = tempfile.mkdtemp()
    depth_dir = os.path.join(tmp, 'depth')
    os.makedirs(depth_dir)
    for f in FRAMES:
        os.symlink(os.path.join(HERE, 'depth_%s.png' % f), os.path.join(depth_dir, f + '.png'))
    _install_stubs(depth_dir)
    import gen_instance_masks
    from monopsr.datasets.kitti import calib_utils, depth_map_utils, instance_utils, obj_utils
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        gen_instance_masks.main()
    finally:
        os.chdir(cwd)
    print()
    data = {'frames': np.array(FRAMES), 'division': np.array('numpy1')}
    for f in FRAMES:
        ref = WRITTEN[f]
        calib = calib_utils.read_frame_calib(os.path.join(KITTI, 'calib', f + '.txt'))
        p2 = np.asarray(calib.p2, np.float64)
        depth = depth_map_utils.read_depth_map(os.path.join(depth_dir, f + '.png'))
        with open(os.path.join(KITTI, 'label_2', f + '.txt')) as fh:
            text = fh.read()
        labels = my_obj.parse_labels(text)
        mine = rs.instance_image(depth, p2, my_iu.instance_box_table(labels))
        assert ref.dtype == np.uint8 and ref.tobytes() == mine.tobytes(), (f, int((ref != mine).sum()))
        Image.fromarray(ref).save(os.path.join(HERE, 'instance_%s.png' % f), optimize=True)
        data['p2_%s' % f] = p2
        data['labels_%s' % f] = np.array(text)
        # the reference's host-side values
        ref_labels = obj_utils.read_labels(os.path.join(KITTI, 'label_2'), f)
        assert len(ref_labels) == len(labels)
        for a, b in zip(ref_labels, labels):
            for k in ('type', 'truncation', 'occlusion', 'alpha', 'x1', 'y1', 'x2', 'y2', 'h', 'w', 'l', 'ry', 'score'):
                va, vb = getattr(a, k), getattr(b, k)
                assert va == vb and type(va) == type(vb), (f, k, va, vb)
            assert a.t.dtype == b.t.dtype and a.t.tobytes() == b.t.tobytes()
        _, mask = obj_utils.filter_labels(ref_labels, classes=['Car'], difficulty=obj_utils.Difficulty.HARD,
                                          truncation=0.3, depth_range=[5, 45])
        _, my_mask = my_obj.filter_labels(labels, classes=['Car'], difficulty=my_obj.Difficulty.HARD, truncation=0.3,
                                          depth_range=[5, 45])
        assert np.array_equal(mask, my_mask)
        data['filter_mask_%s' % f] = np.asarray(mask)
        masks = {}
        for name, kw in (('class', dict(classes=['Car', 'Pedestrian'])), ('easy', dict(difficulty=0)),
                         ('moderate', dict(difficulty=1)), ('height', dict(box_2d_height=25)),
                         ('occlusion', dict(occlusion=1)), ('truncation', dict(truncation=0.5)),
                         ('depth', dict(depth_range=[5, 35]))):
            _, m = obj_utils.filter_labels(ref_labels, **kw)
            _, m2 = my_obj.filter_labels(labels, **kw)
            assert np.array_equal(m, m2), (f, name)
            masks[name] = np.asarray(m)
        for name, m in masks.items():
            data['mask_%s_%s' % (name, f)] = m
        cam_p = p2
        b2 = obj_utils.boxes_2d_from_obj_labels(ref_labels)
        b3 = obj_utils.boxes_3d_from_obj_labels(ref_labels)
        va2 = np.array([obj_utils.get_viewing_angle_box_2d(b, cam_p) for b in b2])
        va3 = np.array([obj_utils.get_viewing_angle_box_3d(b, cam_p) for b in b3])
        assert va2.tobytes() == np.array([my_obj.get_viewing_angle_box_2d(b, cam_p) for b in b2]).tobytes()
        assert va3.tobytes() == np.array([my_obj.get_viewing_angle_box_3d(b, cam_p) for b in b3]).tobytes()
        data['boxes_2d_%s' % f], data['boxes_3d_%s' % f] = b2, b3
        data['view_2d_%s' % f], data['view_3d_%s' % f] = va2, va3
        print('frame', f, ref.shape, 'labels', len(labels), 'instance pixels', int((ref != 255).sum()))
    for c in ('Car', 'Pedestrian', 'Cyclist'):
        data['mean_lwh_%s' % c] = np.array(obj_utils.get_mean_lwh_and_std_dev(c))
        data['prop_cen_z_offset_%s' % c] = np.array(instance_utils.get_prop_cen_z_offset(c))
        assert np.array_equal(data['mean_lwh_%s' % c], np.array(my_obj.get_mean_lwh_and_std_dev(c)))
        assert data['prop_cen_z_offset_%s' % c] == my_iu.get_prop_cen_z_offset(c)
    classes = ['Car', 'Pedestrian', 'Cyclist']
    data['class_index'] = np.array([obj_utils.class_str_to_index(c, classes) for c in classes])
    np.savez_compressed(os.path.join(HERE, 'instance_fixture.npz'), **data)
    print('restatement == reference on %d frames; fixtures written' % len(FRAMES))


if __name__ == '__main__':
    main()
