"""KITTI object labels on the host, with the names and arithmetic of the reference's monopsr/datasets/kitti/obj_utils.py
(read_labels, the filters of :193-345, the viewing angles of :913-983, get_mean_lwh_and_std_dev, class_str_to_index)
and of core/box_3d_encoder's label -> box conversions.  numpy only; nothing here touches the GPU.
"""
import os

import numpy as np

# KITTI difficulty thresholds (easy, moderate, hard)
HEIGHT = (40, 25, 25)
OCCLUSION = (0, 1, 2)
TRUNCATION = (0.15, 0.3, 0.5)


class Difficulty:
    EASY, MODERATE, HARD, ALL = 0, 1, 2, 3
    STR_TO_DIFF_MAPPING = {'easy': EASY, 'moderate': MODERATE, 'hard': HARD, 'all': ALL}

    @staticmethod
    def from_string(difficulty_str):
        return Difficulty.STR_TO_DIFF_MAPPING[difficulty_str]


class ObjectLabel:
    """One label row.  x1 y1 x2 y2, h w l and t are float32 (the reference's astype(np.float32)); truncation,
    occlusion, alpha, ry and score are Python floats."""

    def __init__(self):
        self.type = None
        self.truncation = 0.0
        self.occlusion = 0
        self.alpha = 0.0
        self.x1 = self.y1 = self.x2 = self.y2 = 0.0
        self.h = self.w = self.l = 0.0
        self.t = (0.0, 0.0, 0.0)
        self.ry = 0.0
        self.score = 0.0

    def __repr__(self):
        return '({}, a:{}, t:{} lwh:({:.03f}, {:.03f}, {:.03f}), ry:{:.03f})'.format(
            self.type, self.alpha, self.t, self.l, self.w, self.h, self.ry)


def parse_labels(text):
    """Label file text -> np.ndarray of ObjectLabel (15 columns, or 16 with a score)."""
    rows = [line.split(' ') for line in text.splitlines() if line.strip()]
    if not rows:
        return np.asarray([], dtype=object)
    if any(len(r) != len(rows[0]) for r in rows) or len(rows[0]) not in (15, 16):
        raise ValueError('Invalid label format')
    labels = np.asarray(rows, dtype=str)
    is_results = labels.shape[1] == 16
    obj_list = []
    for row in labels:
        obj = ObjectLabel()
        obj.type = row[0]
        obj.truncation = float(row[1])
        obj.occlusion = float(row[2])
        obj.alpha = float(row[3])
        obj.x1, obj.y1, obj.x2, obj.y2 = row[4:8].astype(np.float32)
        obj.h, obj.w, obj.l = row[8:11].astype(np.float32)
        obj.t = row[11:14].astype(np.float32)
        obj.ry = float(row[14])
        obj.score = float(row[15]) if is_results else 0.0
        obj_list.append(obj)
    out = np.empty(len(obj_list), dtype=object)
    out[:] = obj_list
    return out


def read_labels(label_dir, sample_name):
    """label_dir/<sample_name>.txt -> np.ndarray of ObjectLabel (empty for an empty file)."""
    label_path = os.path.join(label_dir, '{}.txt'.format(sample_name))
    if not os.path.exists(label_path):
        raise FileNotFoundError('Label file could not be found: %s' % label_path)
    with open(label_path) as f:
        return parse_labels(f.read())


def filter_labels_by_class(obj_labels, classes):
    class_mask = [(obj.type in classes) for obj in obj_labels]
    return obj_labels[class_mask], class_mask


def _check_difficulty(obj, difficulty):
    if difficulty == Difficulty.ALL:
        return True
    return ((obj.occlusion <= OCCLUSION[difficulty]) and
            (obj.truncation <= TRUNCATION[difficulty]) and
            (obj.y2 - obj.y1) >= HEIGHT[difficulty])


def filter_labels(obj_labels, classes=None, difficulty=None, box_2d_height=None, occlusion=None, truncation=None,
                  depth_range=None):
    """-> (kept labels, boolean mask).  Class membership; difficulty (occlusion <=, truncation <=, box height >=
    the level's thresholds); box height > box_2d_height; occlusion < occlusion; truncation < truncation;
    depth_range[0] < z < depth_range[1] -- strict or inclusive exactly as obj_utils.py:215-345 writes them."""
    obj_mask = np.full(len(obj_labels), True)
    mask = lambda flags: np.asarray(flags, bool).reshape(-1)  # (an empty label file gives an empty list: float64)
    if classes is not None:
        obj_mask &= mask([(obj.type in classes) for obj in obj_labels])
    if difficulty is not None:
        obj_mask &= mask([_check_difficulty(obj, difficulty) for obj in obj_labels])
    if box_2d_height is not None:
        obj_mask &= mask([(obj.y2 - obj.y1) > box_2d_height for obj in obj_labels])
    if occlusion is not None:
        obj_mask &= mask([obj.occlusion < occlusion for obj in obj_labels])
    if truncation is not None:
        obj_mask &= mask([obj.truncation < truncation for obj in obj_labels])
    if depth_range is not None:
        obj_mask &= mask([depth_range[0] < obj.t[2] < depth_range[1] for obj in obj_labels])
    return obj_labels[obj_mask], obj_mask


class ObjectFilter:
    """obj_filter_config of a dataset config: classes, difficulty_str, box_2d_height, truncation, occlusion,
    depth_range."""

    def __init__(self, classes, difficulty_str='all', box_2d_height=None, truncation=None, occlusion=None,
                 depth_range=None):
        self.classes = list(classes)
        self.difficulty = Difficulty.from_string(difficulty_str)
        self.box_2d_height, self.truncation, self.occlusion = box_2d_height, truncation, occlusion
        self.depth_range = depth_range


def apply_obj_filter(obj_labels, obj_filter):
    return filter_labels(obj_labels, classes=obj_filter.classes, difficulty=obj_filter.difficulty,
                         box_2d_height=obj_filter.box_2d_height, occlusion=obj_filter.occlusion,
                         truncation=obj_filter.truncation, depth_range=obj_filter.depth_range)


def object_label_to_box_2d(obj_label):
    """[y1, x1, y2, x2] float32"""
    return np.asarray([obj_label.y1, obj_label.x1, obj_label.y2, obj_label.x2], np.float32)


def object_label_to_box_3d(obj_label):
    """[x, y, z, l, w, h, ry] float32"""
    box_3d = np.zeros(7, dtype=np.float32)
    box_3d[0:3] = obj_label.t
    box_3d[3:6] = obj_label.l, obj_label.w, obj_label.h
    box_3d[6] = obj_label.ry
    return box_3d


def boxes_2d_from_obj_labels(obj_labels):
    return np.asarray([object_label_to_box_2d(o) for o in obj_labels], np.float32).reshape(-1, 4)


def boxes_3d_from_obj_labels(obj_labels):
    return np.asarray([object_label_to_box_3d(o) for o in obj_labels], np.float32).reshape(-1, 7)


def compute_box_3d_corners(box_3d):
    """(3, 8) corners in the order and arithmetic of obj_utils.compute_box_3d_corners."""
    tx, ty, tz, l, w, h, ry = box_3d
    half_l = l / 2
    half_w = w / 2
    rot = np.array([[+np.cos(ry), 0, +np.sin(ry)],
                    [0, 1, 0],
                    [-np.sin(ry), 0, +np.cos(ry)]])
    x_corners = np.array([half_l, half_l, -half_l, -half_l, half_l, half_l, -half_l, -half_l])
    y_corners = np.array([0, 0, 0, 0, -h, -h, -h, -h])
    z_corners = np.array([half_w, -half_w, -half_w, half_w, half_w, -half_w, -half_w, half_w])
    corners_3d = np.dot(rot, np.array([x_corners, y_corners, z_corners]))
    corners_3d[0, :] = corners_3d[0, :] + tx
    corners_3d[1, :] = corners_3d[1, :] + ty
    corners_3d[2, :] = corners_3d[2, :] + tz
    return np.array(corners_3d)


def box_3d_slab_bounds(box_3d):
    """points_in_box_3d's per-box constants: (u, up0, up1, v, vp0, vp3, w, wp0, wp4); a point p lies inside when
    up1 <= p.u <= up0, vp3 <= p.v <= vp0 and wp4 <= p.w <= wp0."""
    corners_3d = compute_box_3d_corners(box_3d).T
    u = corners_3d[0, :] - corners_3d[1, :]
    v = corners_3d[0, :] - corners_3d[3, :]
    w = corners_3d[0, :] - corners_3d[4, :]
    up0 = np.dot(u, corners_3d[0, :])
    up1 = np.dot(u, corners_3d[1, :])
    vp0 = np.dot(v, corners_3d[0, :])
    vp3 = np.dot(v, corners_3d[3, :])
    wp0 = np.dot(w, corners_3d[0, :])
    wp4 = np.dot(w, corners_3d[4, :])
    return u, up0, up1, v, vp0, vp3, w, wp0, wp4


def get_viewing_angle_box_2d(box_2d, cam_p):
    """atan2((centre_x - cu) / f, 1) of a [y1, x1, y2, x2] box."""
    centre_x = np.mean(box_2d[[1, 3]])
    centre_u = cam_p[0, 2]
    focal_length = cam_p[0, 0]
    return np.arctan2((centre_x - centre_u) / focal_length, 1.0)


def get_viewing_angle_box_3d(box_3d, cam_p=None, version='x_offset'):
    """Viewing angle to the box centroid; 'cam_0' or 'x_offset' (the camera-N frame)."""
    if version == 'cam_0':
        return np.arctan2(box_3d[0], box_3d[2])
    if version == 'x_offset':
        x_offset = -cam_p[0, 3] / cam_p[0, 0]
        box_x_cam = box_3d[0] - x_offset
        return np.arctan2(box_x_cam, box_3d[2])
    raise ValueError('Invalid version', version)


_MEAN_LWH = {
    'Car': ([3.892, 1.619, 1.530], [0.440, 0.106, 0.138]),
    'Pedestrian': ([0.818, 0.628, 1.768], [0.245, 0.122, 0.130]),
    'Cyclist': ([1.771, 0.570, 1.723], [0.153, 0.143, 0.104]),
}


def get_mean_lwh_and_std_dev(class_str):
    if class_str not in _MEAN_LWH:
        raise ValueError('Invalid class_str', class_str)
    mean_lwh, std_dev_lwh = _MEAN_LWH[class_str]
    return list(mean_lwh), list(std_dev_lwh)


def class_str_to_index(class_str, classes):
    """1-based index of class_str in classes (0 is the background class)."""
    if class_str in classes:
        return classes.index(class_str) + 1
    raise ValueError('Invalid class string {}, not in {}'.format(class_str, classes))
