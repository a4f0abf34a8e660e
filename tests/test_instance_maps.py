"""Instance images and ground-truth crops on the host: the restatement against the reference's fixture, the label
helpers, crop-rule known answers, argument errors and the command line.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import instance_restatement as rs
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils as iu, obj_utils

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FIX = np.load(os.path.join(GOLDEN, 'instance_fixture.npz'))
FRAMES = [str(f) for f in FIX['frames']]
ROOT = os.path.dirname(HERE)


def _frame(f):
    depth = depth_map_utils.read_depth_map(os.path.join(GOLDEN, 'depth_%s.png' % f))
    labels = obj_utils.parse_labels(str(FIX['labels_%s' % f]))
    return depth, FIX['p2_%s' % f], labels


@pytest.mark.parametrize('f', FRAMES)
def test_restatement_equals_reference_instance_images(f):
    assert str(FIX['division']) == 'numpy1'
    depth, p2, labels = _frame(f)
    want = np.asarray(Image.open(os.path.join(GOLDEN, 'instance_%s.png' % f)))
    got = rs.instance_image(depth, p2, iu.instance_box_table(labels))
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    assert (want != 255).any()


@pytest.mark.parametrize('f', FRAMES)
def test_label_helpers_equal_reference(f):
    _, p2, labels = _frame(f)
    b2, b3 = obj_utils.boxes_2d_from_obj_labels(labels), obj_utils.boxes_3d_from_obj_labels(labels)
    assert b2.tobytes() == FIX['boxes_2d_%s' % f].tobytes() and b3.tobytes() == FIX['boxes_3d_%s' % f].tobytes()
    va2 = np.array([obj_utils.get_viewing_angle_box_2d(b, p2) for b in b2])
    va3 = np.array([obj_utils.get_viewing_angle_box_3d(b, p2) for b in b3])
    assert va2.tobytes() == FIX['view_2d_%s' % f].tobytes() and va3.tobytes() == FIX['view_3d_%s' % f].tobytes()
    _, m = obj_utils.filter_labels(labels, classes=['Car'], difficulty=obj_utils.Difficulty.HARD, truncation=0.3,
                                   depth_range=[5, 45])
    assert np.array_equal(m, FIX['filter_mask_%s' % f])
    for name, kw in (('class', dict(classes=['Car', 'Pedestrian'])), ('easy', dict(difficulty=0)),
                     ('moderate', dict(difficulty=1)), ('height', dict(box_2d_height=25)),
                     ('occlusion', dict(occlusion=1)), ('truncation', dict(truncation=0.5)),
                     ('depth', dict(depth_range=[5, 35]))):
        assert np.array_equal(obj_utils.filter_labels(labels, **kw)[1], FIX['mask_%s_%s' % (name, f)]), name


def test_class_tables_equal_reference():
    for c in ('Car', 'Pedestrian', 'Cyclist'):
        assert np.array_equal(np.array(obj_utils.get_mean_lwh_and_std_dev(c)), FIX['mean_lwh_%s' % c])
        assert iu.get_prop_cen_z_offset(c) == float(FIX['prop_cen_z_offset_%s' % c])
    classes = ['Car', 'Pedestrian', 'Cyclist']
    assert [obj_utils.class_str_to_index(c, classes) for c in classes] == list(FIX['class_index'])
    with pytest.raises(ValueError):
        obj_utils.class_str_to_index('Van', classes)
    with pytest.raises(ValueError):
        iu.get_prop_cen_z_offset('Van')


def test_training_labels_of_fixture_frames(tmp_path):
    from monopsr_amd.datasets.kitti import kitti_dataset
    (tmp_path / 'label_2').mkdir()
    for f in ('000006', '000002'):
        (tmp_path / 'label_2' / (f + '.txt')).write_text(str(FIX['labels_%s' % f]))
    kept, ids = kitti_dataset.training_labels(str(tmp_path), '000006')
    assert list(ids) == [1, 2, 3] and all(o.type == 'Car' for o in kept)
    _, ids = kitti_dataset.training_labels(str(tmp_path), '000002')
    assert list(ids) == [1]


def test_instance_table_skips_dontcare_and_unknown_types():
    text = ('Car 0.00 0 0.1 10 20 30 40 1.5 1.6 3.9 1.0 1.5 20.0 0.2\n'
            'Blob 0.00 0 0.1 10 20 30 40 1.5 1.6 3.9 1.0 1.5 20.0 0.2\n'
            'Tram 0.00 0 0.1 10 20 30 40 1.5 1.6 3.9 -1.0 1.5 20.0 0.2\n'
            'DontCare -1 -1 -10 1 2 3 4 -1 -1 -1 -1000 -1000 -1000 -10\n')
    t = iu.instance_box_table(obj_utils.parse_labels(text))
    assert t.shape == (2, iu.BOX_STRIDE)
    assert np.array_equal(t[:, 15:19], [[20, 10, 40, 30], [20, 10, 40, 30]])


# ---- crop rules, by hand


def test_box_rounding_is_half_to_even():
    assert [int(rs.round_half_even(v)) for v in (10.5, 11.5, -0.5, 2.4999998)] == [10, 12, 0, 2]


def test_nearest_neighbour_index_rounds_ties_away_from_zero():
    # in 3 -> out 5: scale (3-1)/(5-1) = 0.5, i * 0.5 = 0, .5, 1, 1.5, 2 -> 0, 1, 1, 2, 2
    assert [rs.nn_index(i, 3, 5) for i in range(5)] == [0, 1, 1, 2, 2]
    # out 1: scale in / out, index 0
    assert rs.nn_index(0, 7, 1) == 0
    # clamped to in - 1
    assert rs.nn_index(3, 2, 4) == 1


def _tiny(h=6, w=7):
    depth = (np.arange(h * w, dtype=np.float32).reshape(h, w) + 1) / 4
    inst = np.full((h, w), 255, np.uint8)
    inst[1:, 1:] = 3
    p2 = np.array([[2.0, 0, 3.0, 4.0], [0, 2.0, 2.0, 0], [0, 0, 1, 0]], np.float32)
    return depth, inst, p2


def test_crop_excludes_the_last_row_and_column():
    depth, inst, p2 = _tiny()
    # rows 1:3, columns 2:4 -> roi 2 takes rows 1, 2 and columns 2, 3 (never row 3 / column 4)
    _, glob, valid = rs.instance_xyz_crop(depth, inst, p2, 3, [1, 2, 3, 4], np.zeros(7), 0.0, 2)
    assert np.array_equal(glob[..., 2], depth[1:3, 2:4]) and valid.all()


def test_crop_with_roi_one_and_half_integer_box():
    depth, inst, p2 = _tiny()
    # y 1.5 -> 2, x 2.5 -> 2, y2 4.5 -> 4, x2 5.5 -> 6 (half to even); out 1 takes the top-left source
    _, glob, _ = rs.instance_xyz_crop(depth, inst, p2, 3, [1.5, 2.5, 4.5, 5.5], np.zeros(7), 0.0, 1)
    assert glob[0, 0, 2] == depth[2, 2]
    # pixel centre of the unrounded box: x = (2.5 + 5.5) / 2 = 4, y = 3
    assert glob[0, 0, 0] == np.float32((4.0 - 3.0) * (depth[2, 2] / 2.0))
    assert glob[0, 0, 1] == np.float32((3.0 - 2.0) * (depth[2, 2] / 2.0))


def test_zeroed_entries_keep_the_sign_of_a_multiplication():
    depth, inst, p2 = _tiny()
    # id 7 has no pixels: every depth is masked to 0, valid is 0, coordinates left of cu become -0.0
    loc, glob, valid = rs.instance_xyz_crop(depth, inst, p2, 7, [0, 0, 4, 4], [5, 1, 9, 4, 2, 1.5, 0], 0.3, 4,
                                            rotate_view=False)
    assert not valid.any() and (glob == 0).all() and (loc == 0).all()
    assert np.signbit(loc[..., 0]).all() and np.signbit(loc[..., 2]).all()  # -(x - x_offset), -z translations
    depth[:] = 0.05  # below 0.1: invalid, and x = (xx - cu) * ratio < 0 for xx < cu
    _, glob, valid = rs.instance_xyz_crop(depth, inst, p2, 3, [1, 1, 5, 2], np.zeros(7), 0.0, 1)
    assert not valid.any() and glob[0, 0, 0] == 0 and np.signbit(glob[0, 0, 0])


# ---- argument errors and the command line


def test_host_argument_checks_need_no_gpu():
    from monopsr_amd import _lib
    lib = _lib.lib()
    fi = (ctypes.c_int * 1)(0)
    ii = (ctypes.c_int * 1)(0)
    b2 = (ctypes.c_float * 4)(0, 0, 4, 4)
    args = lambda roi_h, roi_w, n_frames=1, ids=ii, boxes=b2: (1, 1, 1, n_frames, 8, 8, 1, 1, 1, 1, 1, fi, ids, boxes,
                                                               1, roi_h, roi_w, 1, 1, 1, 1, 1, None)
    assert lib.mpsr_instance_xyz_crops(*args(4, 5)) == 1 and b'square' in lib.mpsr_last_error()
    assert lib.mpsr_instance_xyz_crops(*args(4, 4, n_frames=0)) == 1 and b'frame' in lib.mpsr_last_error()
    assert lib.mpsr_instance_xyz_crops(*args(4, 4, ids=(ctypes.c_int * 1)(255))) == 1
    assert b'instance id' in lib.mpsr_last_error()
    for box in ((0, 0, 0.4, 4), (0, 0, 9, 4), (-0.6, 0, 4, 4), (3, 3, 2, 5)):
        assert lib.mpsr_instance_xyz_crops(*args(4, 4, boxes=(ctypes.c_float * 4)(*box))) == 1, box
        assert b'empty or outside' in lib.mpsr_last_error()
    offs = (ctypes.c_longlong * 2)(0, 256)
    assert lib.mpsr_instance_images(1, 1, 8, 8, 1, 1, 1, offs, 1, None) == 1 and b'256 boxes' in lib.mpsr_last_error()


def test_python_argument_checks():
    from monopsr_amd import _lib
    text = '\n'.join(['Car 0.00 0 0.1 10 20 30 40 1.5 1.6 3.9 1.0 1.5 20.0 0.2'] * 256)
    with pytest.raises(_lib.InvalidArgumentError, match='256 boxes'):
        iu.gen_instance_images(np.zeros((1, 4, 4), np.float32), [np.eye(4)[:3]], [obj_utils.parse_labels(text)])
    with pytest.raises(_lib.InvalidArgumentError):
        iu.gen_instance_images(np.zeros((2, 4, 4), np.float32), [np.eye(4)[:3]], [[]])
    with pytest.raises(ValueError):
        obj_utils.parse_labels('Car 0 0 0\n')
    with pytest.raises(ValueError):
        iu.save_instance_image('/nonexistent.png', np.zeros((2, 2), np.float32))


def _cli(*args):
    return subprocess.run([sys.executable, '-m', 'monopsr_amd.datasets.kitti.instance_utils', *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


def test_command_line_help_and_bad_arguments(tmp_path):
    r = _cli('--help')
    assert r.returncode == 0 and 'DEPTH_DIR' in r.stdout.upper() and '--batch' in r.stdout
    r = _cli(str(tmp_path), str(tmp_path), str(tmp_path / 'o'), '--batch', '0')
    assert r.returncode == 2 and '--batch' in r.stderr
    r = _cli(str(tmp_path / 'missing'), str(tmp_path), str(tmp_path / 'o'))
    assert r.returncode == 2 and 'no such directory' in r.stderr
    r = _cli(str(tmp_path))
    assert r.returncode == 2


def test_command_line_rejects_an_image_of_another_size(tmp_path):
    (tmp_path / 'image_2').mkdir()
    (tmp_path / 'depth').mkdir()
    Image.fromarray(np.zeros((5, 6, 3), np.uint8)).save(str(tmp_path / 'image_2' / '000001.png'))
    Image.fromarray(np.zeros((5, 7), np.uint16)).save(str(tmp_path / 'depth' / '000001.png'))
    r = _cli(str(tmp_path), str(tmp_path / 'depth'), str(tmp_path / 'o'))
    assert r.returncode != 0 and 'image_2' in r.stderr
