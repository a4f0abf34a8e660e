"""One KITTI training sample for the trainer: the 'train' branch of the reference's KittiDataset.load_samples
(kitti_dataset.py:260-490), without augmentation, plus the ground-truth maps the reference's graph crops per box
(monopsr_model.py:158-203), built in one mpsr_instance_xyz_crops launch.

    rng = np.random.default_rng(0)
    sample = build_training_sample(split_dir, '000006', depth_dir, instance_dir, rng)
    trainer.step(sample)
"""
import os

import numpy as np
import torch

from monopsr_amd.core import orientation_encoder
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils, obj_utils

# model 000's obj_filter_config (configs/monopsr_model_000.yaml of the reference)
DEFAULT_OBJ_FILTER = dict(difficulty_str='hard', box_2d_height=None, truncation=0.3, occlusion=None,
                          depth_range=[5, 45])


def _read_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def training_labels(split_dir, sample_name, classes=('Car',), obj_filter=None):
    """-> (the labels of label_2/<name>.txt that pass the filter, their instance ids = their rows in the file)."""
    obj_labels = obj_utils.read_labels(os.path.join(split_dir, 'label_2'), sample_name)
    flt = obj_utils.ObjectFilter(list(classes), **(DEFAULT_OBJ_FILTER if obj_filter is None else obj_filter))
    kept, obj_mask = obj_utils.apply_obj_filter(obj_labels, flt)
    return kept, np.arange(len(obj_labels))[obj_mask]


def build_training_sample(split_dir, sample_name, depth_dir, instance_dir, rng, num_boxes=32, classes=('Car',),
                          obj_filter=None, num_alpha_bins=12, alpha_bin_overlap=0.0, map_roi_size=(48, 48),
                          centroid_type='middle', rotate_view=True, device=None):
    """The sample dict MonoPSRModel.build and InstanceTrainer.step read, or None when no label survives the filter.

    Reads image_2/<name>.png (RGB, float32), calib/<name>.txt (P2), label_2/<name>.txt, depth_dir/<name>.png and
    instance_dir/<name>.png.  The labels are filtered by `obj_filter` (keyword arguments of obj_utils.ObjectFilter;
    default DEFAULT_OBJ_FILTER) and `classes`, then oversampled to num_boxes with `rng` (a np.random.Generator; the
    reference draws from the global np.random).

    The instance id of a kept label is its ROW in the label file, as the reference takes it
    (get_instance_mask_list(image, num_all_objs)[obj_mask]).  The instance images number only the labels of
    instance_utils.REQUIRED_CLASSES, so the two agree as long as every DontCare row follows the object rows, which is
    how KITTI writes its label files.

    est_view_angs holds the viewing angles of the 2-D boxes, gt_view_angs those of the 3-D boxes
    (monopsr_model.py:539).  The ground-truth maps are instance_utils.instance_xyz_crops of the boxes with their 2-D
    viewing angles."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    classes = list(classes)
    rgb = _read_rgb(os.path.join(split_dir, 'image_2', sample_name + '.png'))
    image_shape = rgb.shape[0:2]
    cam_p = depth_map_utils.read_calibration(os.path.join(split_dir, 'calib', sample_name + '.txt')).p2
    obj_labels, instance_ids = training_labels(split_dir, sample_name, classes, obj_filter)
    num_objs = len(obj_labels)
    if num_objs < 1:
        return None
    if num_objs > num_boxes:
        raise ValueError('%s keeps %d labels, more than num_boxes = %d' % (sample_name, num_objs, num_boxes))
    instance_image = instance_utils.read_instance_image(os.path.join(instance_dir, sample_name + '.png'))

    oversample_indices = rng.choice(num_objs, num_boxes - num_objs, replace=True)
    oversample_indices = np.hstack([np.arange(0, num_objs), oversample_indices])
    obj_labels = obj_labels[oversample_indices]
    instance_ids = instance_ids[oversample_indices]

    boxes_2d = obj_utils.boxes_2d_from_obj_labels(obj_labels)
    boxes_3d = obj_utils.boxes_3d_from_obj_labels(obj_labels)
    alpha_bins, alpha_regs, valid_bins = zip(*[orientation_encoder.np_orientation_to_angle_bin(
        o.alpha, num_alpha_bins, alpha_bin_overlap) for o in obj_labels])
    view_2d = np.asarray([obj_utils.get_viewing_angle_box_2d(b, cam_p) for b in boxes_2d], np.float32)
    view_3d = np.asarray([obj_utils.get_viewing_angle_box_3d(b, cam_p) for b in boxes_3d], np.float32)
    class_indices = np.asarray([obj_utils.class_str_to_index(o.type, classes) for o in obj_labels],
                               np.int32)[:, None]
    class_strs = [o.type for o in obj_labels]
    prop_cen_z_offset = np.asarray([instance_utils.get_prop_cen_z_offset(c) for c in class_strs], np.float32)
    lwh_means = np.asarray([obj_utils.get_mean_lwh_and_std_dev(c)[0] for c in class_strs], np.float32)
    boxes_2d_norm = boxes_2d / np.tile(image_shape, 2)
    depth_map = depth_map_utils.read_depth_map(os.path.join(depth_dir, sample_name + '.png'))
    if depth_map.shape != image_shape or instance_image.shape != image_shape:
        raise ValueError('%s: image %s, depth map %s, instance image %s' % (sample_name, image_shape, depth_map.shape,
                                                                           instance_image.shape))

    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    with torch.cuda.device(dev):
        local, glob, valid = instance_utils.instance_xyz_crops(
            depth_map[None], instance_image[None], np.asarray(cam_p, np.float32)[None], np.zeros(num_boxes, np.int32),
            instance_ids, boxes_2d, boxes_3d, view_2d, map_roi_size, centroid_type, rotate_view, device=dev)
        return dict(
            rgb_image=t(rgb.astype(np.float32)), boxes_2d=t(boxes_2d), boxes_2d_norm=t(boxes_2d_norm),
            cam_p=t(cam_p), est_view_angs=t(view_2d), class_indices=t(class_indices, torch.int32),
            mean_lwh=t(lwh_means), prop_cen_z_offset=t(prop_cen_z_offset),
            boxes_3d=t(boxes_3d), gt_alpha_bins=t(np.asarray(alpha_bins), torch.int64),
            gt_alpha_regs=t(np.stack(alpha_regs)), gt_alpha_valid_bins=t(np.stack(valid_bins)),
            gt_view_angs=t(view_3d), gt_inst_xyz_maps_local=local, gt_inst_xyz_maps_global=glob,
            gt_valid_mask_maps=valid)
