"""One KITTI training sample for the trainer: the 'train' branch of the reference's KittiDataset.load_samples
(kitti_dataset.py:260-490), without augmentation, plus the ground-truth maps the reference's graph crops per box
(monopsr_model.py:158-203), built in one mpsr_instance_xyz_crops launch.

    rng = np.random.default_rng(0)
    sample = build_training_sample(split_dir, '000006', depth_dir, instance_dir, rng)
    trainer.step(sample)

KittiDataset is the reference's class of that name (kitti_dataset.py:26-556) with the split resident on the card: every
PNG is read once, and a batch is a few small launches without file I/O or a device-to-host copy.

    dataset = KittiDataset(cfg.dataset_config, 'train', seed=0)
    for sample in dataset.next_batch(batch_size=8, shuffle=True):
        trainer.step(sample)
    dataset.check_status()          # once per epoch: reads the crop kernels' device status word
"""
import json
import os

import numpy as np
import torch

from monopsr_amd import _lib
from monopsr_amd.core import orientation_encoder
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils, kitti_aug, mscnn_utils, obj_utils

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


# ------------------------------------------------------------------------------------------------ the resident dataset

BOX_JITTER_TYPES = {None: 0, 'oversample': 1, 'all': 2}  # MPSR_JITTER_*

# the keys of a sample that are rows of the per-label tables, gathered by label row
_ROW_KEYS = ('boxes_2d', 'boxes_2d_norm', 'est_view_angs', 'class_indices', 'mean_lwh', 'prop_cen_z_offset', 'boxes_3d',
             'gt_alpha_bins', 'gt_alpha_regs', 'gt_alpha_valid_bins', 'gt_view_angs')
# the rows of a 'test' sample (kitti_dataset.py:396-471 of the reference): no label, so nothing 3-D
_TEST_ROW_KEYS = ('boxes_2d', 'boxes_2d_norm', 'est_view_angs', 'class_indices', 'mean_lwh', 'prop_cen_z_offset')


def _cfg(config, key, default=None):
    """config.key of a ConfigObj, a dict or any object with attributes; `default` when absent."""
    if config is None:
        return default
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


class EpochIndex:
    """The epoch bookkeeping of the reference's next_batch (kitti_dataset.py:499-556) on sample indices alone: shuffle
    before the first batch, the wrap-around batch that finishes one epoch and starts the next, epochs_completed and
    _index_in_epoch.  The permutations come from np.random.default_rng(seed).permutation (the reference shuffles
    with the global np.random)."""

    def __init__(self, num_samples, seed=0):
        self.num_samples = int(num_samples)
        self.sample_list = np.arange(self.num_samples)
        self._rng = np.random.default_rng(seed)
        self._index_in_epoch = 0
        self.epochs_completed = 0

    def _shuffle_samples(self):
        self.sample_list = self.sample_list[self._rng.permutation(self.num_samples)]

    def next(self, batch_size, shuffle):
        """-> [(samples, epoch), ...]: the batch in order, as one part, or two when it crosses into the next epoch
        (the second part may be empty).  A batch larger than the split is an IndexError in the reference; here it
        raises ValueError before anything changes."""
        batch_size = int(batch_size)
        if batch_size < 1 or batch_size > self.num_samples:
            raise ValueError('batch_size %d not in [1, %d samples]' % (batch_size, self.num_samples))
        start = self._index_in_epoch
        if self.epochs_completed == 0 and start == 0 and shuffle:
            self._shuffle_samples()
        if start + batch_size >= self.num_samples:
            epoch = self.epochs_completed
            self.epochs_completed += 1
            rest_num_examples = self.num_samples - start
            parts = [(self.sample_list[start:self.num_samples].copy(), epoch)]
            if shuffle:
                self._shuffle_samples()
            self._index_in_epoch = batch_size - rest_num_examples
            parts.append((self.sample_list[0:self._index_in_epoch].copy(), epoch + 1))
            return parts
        self._index_in_epoch += batch_size
        return [(self.sample_list[start:self._index_in_epoch].copy(), self.epochs_completed)]

    def state_dict(self):
        """Where the epoch bookkeeping stands, as values np.savez stores without pickling: the bit generator's state
        (JSON: PCG64's words are 128-bit integers), sample_list, _index_in_epoch and epochs_completed.  An object that
        loads it draws the batches this one draws from here on."""
        return {'num_samples': np.asarray(self.num_samples, np.int64),
                'bit_generator_state': np.asarray(json.dumps(self._rng.bit_generator.state)),
                'sample_list': np.asarray(self.sample_list, np.int64).copy(),
                'index_in_epoch': np.asarray(self._index_in_epoch, np.int64),
                'epochs_completed': np.asarray(self.epochs_completed, np.int64)}

    def load_state_dict(self, state):
        """Take over a state_dict() of an index over the same number of samples; a ValueError changes nothing."""
        num_samples = int(state['num_samples'])
        sample_list = np.asarray(state['sample_list'], np.int64).reshape(-1)
        index_in_epoch, epochs_completed = int(state['index_in_epoch']), int(state['epochs_completed'])
        if num_samples != self.num_samples:
            raise ValueError('the state is of %d samples, this index of %d' % (num_samples, self.num_samples))
        if not np.array_equal(np.sort(sample_list), np.arange(self.num_samples)):
            raise ValueError('sample_list of the state is not a permutation of the %d samples' % self.num_samples)
        if not 0 <= index_in_epoch <= self.num_samples or epochs_completed < 0:
            raise ValueError('the state stands at sample %d of epoch %d' % (index_in_epoch, epochs_completed))
        rng_state = json.loads(str(np.asarray(state['bit_generator_state'])[()]))
        if rng_state.get('bit_generator') != type(self._rng.bit_generator).__name__:
            raise ValueError('the state is of a %s bit generator, this index draws from %s' % (
                rng_state.get('bit_generator'), type(self._rng.bit_generator).__name__))
        self._rng.bit_generator.state = rng_state
        self.sample_list = sample_list.copy()
        self._index_in_epoch, self.epochs_completed = index_in_epoch, epochs_completed


class _Group:
    """The frames of one image size: (F, H, W, 3) uint8 RGB, (F, H, W) float32 depth, (F, H, W) uint8 instance images,
    (F, 3, 4) float32 P2."""

    def __init__(self, shape):
        self.shape = shape
        self.frames = []  # resident frame indices, in load order
        self.rgb = self.depth = self.inst = self.p2 = None


class KittiDataset:
    """The reference's KittiDataset with the split resident on the GPU.

    dataset_config holds the reference's keys (configs/monopsr_model_000.yaml): dataset_dir, data_split,
    data_split_dir, num_boxes, classes, oversample, num_alpha_bins, alpha_bin_overlap, obj_filter_config,
    aug_config.{use_image_aug, image_noise, box_jitter_type}, use_mscnn_detections, depth_version, instance_version.
    Depth maps are read from <data_split_dir>/depth_2_<depth_version>/<name>.png and instance images from
    <data_split_dir>/instance_2_<instance_version>/<name>.png unless depth_dir / instance_dir name other directories.

    Frames that keep no label are left out of sample_list and counted in num_skipped (the reference returns None for
    them and its model draws again).  A frame's sample depends on (seed, epoch, the frame's index in the split file)
    only.  Unsupported recipes raise ValueError naming the option; see DESIGN.md section 7.4 for what is kept.

    aug_config.use_image_aug: True (the reference's apply_image_noise on every 'train' frame) needs image_noise (the
    argument, or aug_config.image_noise): 'reference' for what that function does (only the last stage that fires is
    seen, and its swap copies B into G) or 'composed' for what it describes (the fired stages one after the other, a
    true exchange of G and B).  rgb_image is then made by one mpsr_image_noise launch per image size and each sample
    gains image_noise_stages (an int32 scalar on the device, bit k = kitti_aug.IMAGE_NOISE_STAGES[k] fired).  'val'
    and 'test' never add noise.

    The two evaluation recipes need mscnn_label_dir (the argument, or the config key of that name): the directory of
    MSCNN detections in KITTI label format, one file per frame of the split.  'val' with use_mscnn_detections merges
    them into the labels at load (one mpsr_merge_detections launch); 'test' builds its samples
    from the detection files alone, always oversampled, and reads no label, depth map or instance image.  Samples of
    both carry label_scores."""

    def __init__(self, dataset_config, train_val_test, device=None, seed=0, max_resident_bytes=None, depth_dir=None,
                 instance_dir=None, map_roi_size=(48, 48), centroid_type=None, rotate_view=True, log=None,
                 mscnn_label_dir=None, image_noise=None):
        self.dataset_config = dataset_config
        self.train_val_test = train_val_test
        self.seed = int(seed)
        self.name = _cfg(dataset_config, 'name', 'kitti')
        self.data_split = _cfg(dataset_config, 'data_split', 'train')
        self.num_boxes = int(_cfg(dataset_config, 'num_boxes', 32))
        self.num_alpha_bins = int(_cfg(dataset_config, 'num_alpha_bins', 12))
        self.alpha_bin_overlap = float(_cfg(dataset_config, 'alpha_bin_overlap', 0.0))
        self.centroid_type = centroid_type or _cfg(dataset_config, 'centroid_type', 'middle')
        self.map_roi_size = (int(map_roi_size[0]), int(map_roi_size[1]))
        self.rotate_view = bool(rotate_view)
        self.classes = list(_cfg(dataset_config, 'classes', ['Car']))
        self.num_classes = len(self.classes)
        self.oversample = bool(_cfg(dataset_config, 'oversample', True))
        self.use_mscnn_detections = bool(_cfg(dataset_config, 'use_mscnn_detections', False))
        self.aug_config = _cfg(dataset_config, 'aug_config')
        self.box_jitter_type = _cfg(self.aug_config, 'box_jitter_type')
        self.use_image_aug = bool(_cfg(self.aug_config, 'use_image_aug', False))
        self.image_noise = image_noise if image_noise is not None else _cfg(self.aug_config, 'image_noise')
        self.depth_version = _cfg(dataset_config, 'depth_version', 'multiscale')
        self.instance_version = _cfg(dataset_config, 'instance_version', 'depth_2_multiscale')
        self.iou_threshold_min = 0.7  # kitti_dataset.py:327-349
        self.mscnn_label_dir = mscnn_label_dir or _cfg(dataset_config, 'mscnn_label_dir')
        self.has_kitti_labels = bool(_cfg(dataset_config, 'has_kitti_labels', train_val_test != 'test'))
        self._check_options()
        self.is_test = self.train_val_test == 'test'
        self.merges_mscnn = self.train_val_test == 'val' and self.use_mscnn_detections
        self.mscnn_merge_min_iou = mscnn_utils.MIN_IOU.get(self.classes[0], 0.5)
        if self.is_test:
            self.oversample = True  # kitti_dataset.py:412-416
        self._row_keys = _TEST_ROW_KEYS if self.is_test else _ROW_KEYS
        if self.is_test or self.merges_mscnn:
            self._row_keys = self._row_keys + ('label_scores',)

        flt = _cfg(dataset_config, 'obj_filter_config')
        self.obj_filter = {k: _cfg(flt, k, v) for k, v in DEFAULT_OBJ_FILTER.items()}
        if self.obj_filter['depth_range'] is not None:
            self.obj_filter['depth_range'] = list(self.obj_filter['depth_range'])

        self.dataset_dir = os.path.expanduser(_cfg(dataset_config, 'dataset_dir', '~/Kitti/object'))
        if not os.path.exists(self.dataset_dir):
            raise FileNotFoundError('Dataset path does not exist: {}'.format(self.dataset_dir))
        set_file = os.path.join(self.dataset_dir, self.data_split + '.txt')
        if not os.path.isfile(set_file):
            splits = sorted(f[:-4] for f in os.listdir(self.dataset_dir) if f.endswith('.txt') and f != 'readme.txt')
            raise ValueError('Invalid data split: {}, possible_splits: {}'.format(self.data_split, splits))
        self.data_split_dir = os.path.join(self.dataset_dir, _cfg(dataset_config, 'data_split_dir', 'training'))
        if not os.path.isdir(self.data_split_dir):
            raise ValueError('Invalid data split dir: {}'.format(self.data_split_dir))
        self.rgb_image_dir = os.path.join(self.data_split_dir, 'image_2')
        self.calib_dir = os.path.join(self.data_split_dir, 'calib')
        self.kitti_label_dir = os.path.join(self.data_split_dir, 'label_2')
        self.depth_dir = depth_dir or os.path.join(self.data_split_dir, 'depth_2_{}'.format(self.depth_version))
        self.instance_dir = instance_dir or os.path.join(self.data_split_dir,
                                                         'instance_2_{}'.format(self.instance_version))
        with open(set_file) as f:
            self.split_sample_names = [line for line in f.read().splitlines() if line.strip()]

        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_resident_bytes = max_resident_bytes
        self.resident_bytes = 0
        self.num_skipped = 0
        self._load(log)
        self._epochs = EpochIndex(self.num_samples, self.seed)

    # ---- options

    def _check_options(self):
        if self.train_val_test == 'test' and not self.mscnn_label_dir:
            raise ValueError("train_val_test = 'test' builds its samples from MSCNN detections: give mscnn_label_dir")
        if self.train_val_test not in ('train', 'val', 'test'):
            raise ValueError('Invalid run mode', self.train_val_test)
        if self.num_classes > 1:
            raise NotImplementedError('Number of classes must be 1')
        if self.train_val_test == 'val' and self.use_mscnn_detections and not self.mscnn_label_dir:
            raise ValueError("use_mscnn_detections = True in 'val' mode merges MSCNN boxes into the labels: give "
                             "mscnn_label_dir, or set it to False to validate on KITTI's boxes")
        self.jitter_mode = 0
        self.image_noise_mode = 0  # MPSR_IMAGE_NOISE_*; 0: the frames are gathered and converted as they are
        if self.train_val_test == 'train':
            if self.use_image_aug:
                image_noise = getattr(self, 'image_noise', None)
                if image_noise is None:
                    raise ValueError(
                        "aug_config.use_image_aug = True needs image_noise: the reference's apply_image_noise does not "
                        "do what it describes, so choose 'reference' (what it does: only the last stage that fires is "
                        "seen, and its swap copies B into G) or 'composed' (what it describes: the fired stages act "
                        "one after the other, and the swap exchanges G and B)")
                self.image_noise_mode = kitti_aug.image_noise_mode(image_noise)
            if self.box_jitter_type == 'oversample_gt':
                raise ValueError("aug_config.box_jitter_type = 'oversample_gt' is not built")
            if self.box_jitter_type not in BOX_JITTER_TYPES:
                raise ValueError('Invalid box_jitter_type', self.box_jitter_type)
            if self.box_jitter_type == 'oversample' and not self.oversample:
                raise ValueError('Must oversample object labels to use {} box jitter type'.format(
                    self.box_jitter_type))
            self.jitter_mode = BOX_JITTER_TYPES[self.box_jitter_type]

    # ---- loading

    def _reserve(self, nbytes):
        if self.max_resident_bytes is not None and self.resident_bytes + nbytes > self.max_resident_bytes:
            raise MemoryError('KittiDataset: the split needs %d more bytes on the device, %d are resident and '
                              'max_resident_bytes is %d' % (nbytes, self.resident_bytes, self.max_resident_bytes))
        self.resident_bytes += nbytes

    def _upload(self, array, dtype):
        t = torch.as_tensor(np.ascontiguousarray(array), dtype=dtype)
        self._reserve(t.numel() * t.element_size())
        return t.to(self.device)

    def _label_rows(self, obj_labels, cam_p, image_shape):
        """The per-label rows of one frame, with the functions and in the order of build_training_sample."""
        boxes_2d = obj_utils.boxes_2d_from_obj_labels(obj_labels)
        label_boxes = np.asarray([[float(o.x1), float(o.y1), float(o.x2), float(o.y2)] for o in obj_labels],
                                 np.float64)
        label_scores = np.asarray([o.score for o in obj_labels], np.float32)
        if self.is_test:
            class_strs = [o.type for o in obj_labels]
            return dict(
                boxes_2d=boxes_2d, boxes_2d_norm=boxes_2d / np.tile(image_shape, 2),
                est_view_angs=np.asarray([obj_utils.get_viewing_angle_box_2d(b, cam_p) for b in boxes_2d], np.float32),
                class_indices=np.asarray([obj_utils.class_str_to_index(c, self.classes) for c in class_strs],
                                         np.int32)[:, None],
                mean_lwh=np.asarray([obj_utils.get_mean_lwh_and_std_dev(c)[0] for c in class_strs], np.float32),
                prop_cen_z_offset=np.asarray([instance_utils.get_prop_cen_z_offset(c) for c in class_strs],
                                             np.float32),
                label_boxes=label_boxes, label_scores=label_scores)
        boxes_3d = obj_utils.boxes_3d_from_obj_labels(obj_labels)
        alpha_bins, alpha_regs, valid_bins = zip(*[orientation_encoder.np_orientation_to_angle_bin(
            o.alpha, self.num_alpha_bins, self.alpha_bin_overlap) for o in obj_labels])
        class_strs = [o.type for o in obj_labels]
        return dict(
            boxes_2d=boxes_2d, boxes_2d_norm=boxes_2d / np.tile(image_shape, 2),
            est_view_angs=np.asarray([obj_utils.get_viewing_angle_box_2d(b, cam_p) for b in boxes_2d], np.float32),
            class_indices=np.asarray([obj_utils.class_str_to_index(c, self.classes) for c in class_strs],
                                     np.int32)[:, None],
            mean_lwh=np.asarray([obj_utils.get_mean_lwh_and_std_dev(c)[0] for c in class_strs], np.float32),
            prop_cen_z_offset=np.asarray([instance_utils.get_prop_cen_z_offset(c) for c in class_strs], np.float32),
            boxes_3d=boxes_3d, gt_alpha_bins=np.asarray(alpha_bins), gt_alpha_regs=np.stack(alpha_regs),
            gt_alpha_valid_bins=np.stack(valid_bins),
            gt_view_angs=np.asarray([obj_utils.get_viewing_angle_box_3d(b, cam_p) for b in boxes_3d], np.float32),
            label_boxes=label_boxes, label_scores=label_scores)

    def _split_labels(self):
        """Per frame of the split: (the labels its samples are built from, their rows in the label file)."""
        names = self.split_sample_names
        if self.is_test:
            # just the classes (kitti_dataset.py:56-65, 404-410)
            flt = obj_utils.ObjectFilter(self.classes, 'all')
            out = []
            for name in names:
                labels = obj_utils.read_labels(self.mscnn_label_dir, name)
                kept, mask = obj_utils.apply_obj_filter(labels, flt)
                out.append((kept, np.arange(len(labels))[mask]))
            return out
        if not self.merges_mscnn:
            return [training_labels(self.data_split_dir, name, self.classes, self.obj_filter) for name in names]
        flt = obj_utils.ObjectFilter(self.classes, **self.obj_filter)
        kitti = [obj_utils.read_labels(self.kitti_label_dir, name) for name in names]
        mscnn = [obj_utils.read_labels(self.mscnn_label_dir, name) for name in names]
        ka, ma = [mscnn_utils.label_arrays(k) for k in kitti], [mscnn_utils.label_arrays(m) for m in mscnn]
        boxes, scores, _ = mscnn_utils.merge_frames([a[0] for a in ka], [a[1] for a in ka], [a[0] for a in ma],
                                                    [a[2] for a in ma], self.mscnn_merge_min_iou, 'distance',
                                                    device=self.device)
        out = []
        for f in range(len(names)):
            merged = mscnn_utils.merged_obj_labels(kitti[f], boxes[f], scores[f])
            kept, mask = obj_utils.apply_obj_filter(merged, flt)
            # the reference's second check: the original labels must keep something under the same filter
            if len(kept) and not len(obj_utils.apply_obj_filter(kitti[f], flt)[0]):
                kept, mask = kept[:0], np.zeros(len(merged), bool)
            out.append((kept, np.arange(len(merged))[mask]))
        return out

    def _load(self, log):
        # pass 1, host only: labels, calibration and image sizes of every frame; what the split needs on the card
        frames, rows, groups = [], [], {}
        split_labels = self._split_labels()
        for split_index, name in enumerate(self.split_sample_names):
            obj_labels, instance_ids = split_labels[split_index]
            if len(obj_labels) < 1:
                self.num_skipped += 1
                continue
            if self.oversample and len(obj_labels) > self.num_boxes:
                raise ValueError('%s keeps %d labels, more than num_boxes = %d' % (name, len(obj_labels),
                                                                                    self.num_boxes))
            if not self.is_test and instance_ids.max() > 254:
                raise ValueError('%s: label row %d has no instance id (0..254)' % (name, instance_ids.max()))
            shape = depth_map_utils.image_shape(os.path.join(self.rgb_image_dir, name + '.png'))
            cam_p = depth_map_utils.read_calibration(os.path.join(self.calib_dir, name + '.txt')).p2
            row = self._label_rows(obj_labels, cam_p, shape)
            row['instance_id'] = instance_ids.astype(np.int32)
            if self.train_val_test == 'val':
                # the KITTI label rows themselves: with MSCNN merging obj_labels carry the detections' boxes, and
                # instance_ids are the rows of the label file either way (_split_labels)
                kitti = obj_utils.read_labels(self.kitti_label_dir, name)[instance_ids]
                row['label_info'] = np.asarray([[o.truncation, o.occlusion, o.x1, o.y1, o.x2, o.y2] for o in kitti],
                                               np.float32).reshape(-1, 6)
            group = groups.setdefault(tuple(shape), _Group(tuple(shape)))
            frames.append(dict(name=name, split_index=split_index, shape=tuple(shape), cam_p=np.asarray(cam_p),
                               num_objs=len(obj_labels), group=group, local=len(group.frames)))
            group.frames.append(len(frames) - 1)
            rows.append(row)
        if not frames:
            raise ValueError('no frame of split %r keeps a label' % self.data_split)
        pixel_bytes = 3 if self.is_test else 3 + 4 + 1
        need = sum(len(g.frames) * g.shape[0] * g.shape[1] * pixel_bytes for g in groups.values())
        if self.max_resident_bytes is not None and need > self.max_resident_bytes:
            raise MemoryError('KittiDataset: the images of split %r need %d bytes on the device, max_resident_bytes is '
                              '%d' % (self.data_split, need, self.max_resident_bytes))

        # pass 2: the images, one frame on the host at a time
        self._frames = frames
        self._groups = list(groups.values())
        self.num_samples = len(frames)
        with torch.cuda.device(self.device):
            for gi, g in enumerate(self._groups):
                g.index = gi
                h, w = g.shape
                nf = len(g.frames)
                self._reserve(nf * h * w * pixel_bytes + nf * 48)
                g.rgb = torch.empty((nf, h, w, 3), dtype=torch.uint8, device=self.device)
                if not self.is_test:
                    g.depth = torch.empty((nf, h, w), dtype=torch.float32, device=self.device)
                    g.inst = torch.empty((nf, h, w), dtype=torch.uint8, device=self.device)
                g.p2 = torch.as_tensor(np.stack([frames[r]['cam_p'] for r in g.frames]).astype(np.float32)) \
                    .to(self.device)
                for k, r in enumerate(g.frames):
                    name = frames[r]['name']
                    rgb = _read_rgb(os.path.join(self.rgb_image_dir, name + '.png'))
                    if self.is_test:
                        if rgb.shape[0:2] != g.shape:
                            raise ValueError('%s: image %s, expected %s' % (name, rgb.shape[0:2], g.shape))
                        g.rgb[k].copy_(torch.from_numpy(np.ascontiguousarray(rgb)))
                        continue
                    depth = depth_map_utils.read_depth_map(os.path.join(self.depth_dir, name + '.png'))
                    inst = instance_utils.read_instance_image(os.path.join(self.instance_dir, name + '.png'))
                    if rgb.shape[0:2] != g.shape or depth.shape != g.shape or inst.shape != g.shape:
                        raise ValueError('%s: image %s, depth map %s, instance image %s' % (
                            name, rgb.shape[0:2], depth.shape, inst.shape))
                    g.rgb[k].copy_(torch.from_numpy(np.ascontiguousarray(rgb)))
                    g.depth[k].copy_(torch.from_numpy(np.ascontiguousarray(depth)))
                    g.inst[k].copy_(torch.from_numpy(np.ascontiguousarray(inst)))
                    if log and (k + 1) % 256 == 0:
                        log('%d x %d: %d / %d frames' % (h, w, k + 1, nf))

            # the per-label and per-frame tables
            cat = lambda k: np.concatenate([row[k] for row in rows])
            f32, i32 = torch.float32, torch.int32
            self._rows = {k: self._upload(cat(k), torch.int64 if k == 'gt_alpha_bins' else
                                          i32 if k == 'class_indices' else f32) for k in self._row_keys}
            self._instance_id = self._upload(cat('instance_id'), i32)
            self._label_boxes = self._upload(cat('label_boxes'), torch.float64)
            self._num_objs_host = np.asarray([f['num_objs'] for f in frames], np.int32)
            offsets = np.concatenate([[0], np.cumsum(self._num_objs_host)[:-1]]).astype(np.int64)
            self._local_host = np.asarray([f['local'] for f in frames], np.int32)
            self._group_host = np.asarray([f['group'].index for f in frames], np.int32)
            self._num_objs = self._upload(self._num_objs_host, i32)
            self._label_offset = self._upload(offsets, torch.int64)
            self._split_index = self._upload([f['split_index'] for f in frames], i32)
            self._frame_local = self._upload(self._local_host, i32)
            self._image_hw = self._upload([f['shape'] for f in frames], i32)
            self._p00_p02 = self._upload([[f['cam_p'][0, 0], f['cam_p'][0, 2]] for f in frames], torch.float64)
            self._cam_p = self._upload(np.stack([f['cam_p'] for f in frames]), f32)
            self._status = torch.zeros(2, dtype=i32, device=self.device)
            # frame_label_info's table: kept on the host, uploaded (and reserved) when the method is first called
            self._label_info_host = cat('label_info') if self.train_val_test == 'val' else None
            self._label_info = None

    # ---- the reference's interface

    @property
    def sample_list(self):
        """The frames (indices into sample_names) in the order of the current epoch."""
        return self._epochs.sample_list

    @property
    def epochs_completed(self):
        return self._epochs.epochs_completed

    @property
    def _index_in_epoch(self):
        return self._epochs._index_in_epoch

    @property
    def sample_names(self):
        """The names of the frames that keep a label, in split-file order; sample_list indexes it."""
        return [f['name'] for f in self._frames]

    def frame_info(self, sample_name):
        """(cam_p (3,4), (image_w, image_h)) of a kept frame, as evaluator_utils.export_kitti_labels asks for them."""
        for f in self._frames:
            if f['name'] == sample_name:
                return f['cam_p'], (f['shape'][1], f['shape'][0])
        raise KeyError(sample_name)

    def frame_calibrations(self):
        """(P2 (F,12) float64, image sizes (F,2) int32 [width, height]) of the kept frames, in sample_names' order."""
        return (np.ascontiguousarray(np.stack([f['cam_p'] for f in self._frames]).astype(np.float64).reshape(-1, 12)),
                np.asarray([[f['shape'][1], f['shape'][0]] for f in self._frames], np.int32))

    def get_sample_names(self):
        return [self._frames[r]['name'] for r in self.sample_list]

    def next_batch(self, batch_size, shuffle):
        """The next batch_size samples: a list of dicts with the keys of build_training_sample plus sample_name,
        num_objs, oversample_indices and jitter_trials (and image_noise_stages with use_image_aug).  The batch that
        finishes an epoch takes its remaining samples from the next one (kitti_dataset.py:504-556)."""
        samples = []
        for frames, epoch in self._epochs.next(batch_size, shuffle):
            samples.extend(self._build(frames, epoch))
        return samples

    def state_dict(self):
        """The position in the split: EpochIndex.state_dict plus the seed and what identifies the split (its name and
        the names of the frames that keep a label).  A sample depends on (seed, epoch, frame) only, so a dataset that
        loads this continues with the batches this one would have built."""
        state = self._epochs.state_dict()
        state.update(seed=np.asarray(self.seed, np.int64), data_split=np.asarray(self.data_split),
                     sample_names=np.asarray(self.sample_names))
        return state

    def load_state_dict(self, state):
        """Continue where a state_dict() of a dataset over the same split stood (its seed included); a state whose
        num_samples or split names differ is a ValueError and changes nothing."""
        if int(state['num_samples']) != self.num_samples:
            raise ValueError('the state is of %d samples, this split holds %d' % (int(state['num_samples']),
                                                                                 self.num_samples))
        names = [str(n) for n in np.asarray(state['sample_names']).reshape(-1)]
        if str(np.asarray(state['data_split'])[()]) != self.data_split or names != self.sample_names:
            raise ValueError("the state is of split '%s' (%d frames), not of this '%s' split's frames" % (
                str(np.asarray(state['data_split'])[()]), len(names), self.data_split))
        self._epochs.load_state_dict(state)
        self.seed = int(state['seed'])

    def get_sample_dict(self, indices, epoch=None):
        """The samples of sample_list[indices] as they are in `epoch` (default: the current one); the bookkeeping of
        next_batch is not touched."""
        epoch = self.epochs_completed if epoch is None else int(epoch)
        return self._build(self.sample_list[np.asarray(indices, np.int64).reshape(-1)], epoch)

    def status(self):
        """(flags, count) of the crop launches' device status word since the last reset: the OR of
        MPSR_CROP_BAD_* and the number of boxes reported.  Reading it synchronises."""
        flags, count = self._status.cpu().tolist()
        return flags, count

    def check_status(self):
        """Raise if a crop launch met a box outside its image, an empty box or a bad id since the last call."""
        flags, count = self.status()
        if flags:
            self._status.zero_()
            raise _lib.InvalidArgumentError('KittiDataset: %d boxes were rejected by the crop kernel (flags 0x%x: '
                                            '1 frame, 2 instance id, 4 not finite, 8 empty or outside the image)'
                                            % (count, flags))

    # ---- ground truth of whole frames

    def _label_instance_ids(self, label_row):
        """The value each label row (int64, on the device) has in its frame's instance image: what the crop kernel is
        given for a slot (_build) and what a reconstruction is scored against (frame_ground_truth)."""
        return self._instance_id.index_select(0, label_row)

    def frame_ground_truth(self, rows):
        """The ground truth of whole frames, for rows of the frame tables (indices into sample_names: the `rows` an
        Evaluator chunk hook receives).  -> one dict per frame: depth_map (h, w) float32 and instance_image (h, w)
        uint8, views of the resident stacks (no copy), and instance_ids (num_objs,) int32 on the device: the value of
        the frame's k-th object in instance_image, i.e. the id _build hands to the crop kernel for the frame's slot k
        (k < num_objs: the slots that are not oversampled).  'test' mode has no ground truth: ValueError."""
        if self.is_test:
            raise ValueError("frame_ground_truth: a 'test'-mode dataset reads no depth map or instance image")
        rows = np.asarray(rows, np.int64).reshape(-1)
        if len(rows) and (rows.min() < 0 or rows.max() >= self.num_samples):
            raise IndexError('frame index out of range [0, %d)' % self.num_samples)
        starts = np.concatenate([[0], np.cumsum(self._num_objs_host)]).astype(np.int64)
        out = []
        with torch.cuda.device(self.device):
            for r in rows:
                g, local = self._groups[self._group_host[r]], int(self._local_host[r])
                label_row = torch.arange(int(starts[r]), int(starts[r + 1]), dtype=torch.int64, device=self.device)
                out.append(dict(depth_map=g.depth[local], instance_image=g.inst[local],
                                instance_ids=self._label_instance_ids(label_row)))
        return out

    def frame_label_info(self, rows):
        """The KITTI label rows of whole frames ('val' mode), for rows of the frame tables as frame_ground_truth takes
        them.  -> one (num_objs, 6) float32 device tensor per frame, [truncation, occlusion, x1, y1, x2, y2] of the
        label-file row of each kept object: with use_mscnn_detections the 2-D box is the label's own, not the
        detection that replaced it in boxes_2d.  The table is uploaded on the first call."""
        if self._label_info_host is None:
            raise ValueError("frame_label_info: only a 'val'-mode dataset keeps its KITTI label rows, this one is %r"
                             % (self.train_val_test,))
        rows = np.asarray(rows, np.int64).reshape(-1)
        if len(rows) and (rows.min() < 0 or rows.max() >= self.num_samples):
            raise IndexError('frame index out of range [0, %d)' % self.num_samples)
        if self._label_info is None:
            with torch.cuda.device(self.device):
                self._label_info = self._upload(self._label_info_host, torch.float32)
        starts = np.concatenate([[0], np.cumsum(self._num_objs_host)]).astype(np.int64)
        return [self._label_info[int(starts[r]):int(starts[r + 1])] for r in rows]

    # ---- one batch

    def _build(self, frames, epoch):
        frames = np.asarray(frames, np.int64).reshape(-1)
        nb = len(frames)
        if nb == 0:
            return []
        if frames.min() < 0 or frames.max() >= self.num_samples:
            raise IndexError('sample index out of range [0, %d)' % self.num_samples)
        dev = self.device
        # frames of one image size side by side: one crop launch per size
        order = np.argsort(self._group_host[frames], kind='stable')
        sorted_frames = frames[order]
        nslots = np.full(nb, self.num_boxes, np.int64) if self.oversample else \
            self._num_objs_host[sorted_frames].astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(nslots)])
        n = int(starts[-1])
        slot_s = np.arange(n) - np.repeat(starts[:-1], nslots)
        meta_host = np.concatenate([np.repeat(sorted_frames, nslots), slot_s, sorted_frames,
                                    self._local_host[sorted_frames]]).astype(np.int32)
        f32, i32 = torch.float32, torch.int32
        roi_h, roi_w = self.map_roi_size
        L = _lib.lib()
        with torch.cuda.device(dev):
            # (pinned: the copy is asynchronous and the caching host allocator keeps the buffer until it is done)
            meta = torch.from_numpy(meta_host).pin_memory().to(dev, non_blocking=True)
            slot_frame, slot_sd = meta[0:n], meta[n:2 * n]
            batch_frames, batch_local = meta[2 * n:2 * n + nb].long(), meta[2 * n + nb:].long()
            label_row = torch.empty(n, dtype=torch.int64, device=dev)
            ints = torch.empty(6 * n, dtype=i32, device=dev)  # one allocation for the five per-slot int32 outputs
            over_idx, flag, slot_hw = ints[0:n], ints[n:2 * n], ints[2 * n:4 * n].view(n, 2)
            slot_split, slot_local = ints[4 * n:5 * n], ints[5 * n:6 * n]
            doubles = torch.empty(6 * n, dtype=torch.float64, device=dev)
            boxes_xyxy, slot_p = doubles[0:4 * n].view(n, 4), doubles[4 * n:6 * n].view(n, 2)  # label boxes; P00, P02
            stream = _lib.stream()
            _lib.check(L.mpsr_sample_slots(
                _lib.ptr(slot_frame), _lib.ptr(slot_sd), n, _lib.ptr(self._num_objs), _lib.ptr(self._label_offset),
                _lib.ptr(self._split_index), _lib.ptr(self._frame_local), _lib.ptr(self._image_hw),
                _lib.ptr(self._p00_p02), _lib.ptr(self._label_boxes), self.num_samples,
                self.seed & 0xFFFFFFFFFFFFFFFF, int(epoch), self.jitter_mode, _lib.ptr(label_row), _lib.ptr(over_idx),
                _lib.ptr(flag), _lib.ptr(boxes_xyxy), _lib.ptr(slot_hw), _lib.ptr(slot_p), _lib.ptr(slot_split),
                _lib.ptr(slot_local), stream))
            rows = {k: t.index_select(0, label_row) for k, t in self._rows.items()}
            instance_id = self._label_instance_ids(label_row)
            if self.jitter_mode:
                trials = torch.empty(n, dtype=i32, device=dev)
                out_xyxy = torch.empty((n, 4), dtype=torch.float64, device=dev)
                _lib.check(L.mpsr_jitter_boxes_2d(
                    _lib.ptr(boxes_xyxy), _lib.ptr(flag), _lib.ptr(slot_hw), _lib.ptr(slot_p), _lib.ptr(slot_split),
                    _lib.ptr(slot_sd), n, self.seed & 0xFFFFFFFFFFFFFFFF, int(epoch), self.iou_threshold_min,
                    kitti_aug.MAX_TRIALS, 0, _lib.ptr(out_xyxy), _lib.ptr(rows['boxes_2d']),
                    _lib.ptr(rows['boxes_2d_norm']), _lib.ptr(rows['est_view_angs']), _lib.ptr(trials), stream))
            else:
                trials = torch.zeros(n, dtype=i32, device=dev)
            if not self.is_test:
                local = torch.empty((n, roi_h, roi_w, 3), dtype=f32, device=dev)
                glob = torch.empty((n, roi_h, roi_w, 3), dtype=f32, device=dev)
                valid = torch.empty((n, roi_h, roi_w, 1), dtype=f32, device=dev)
            rgb = [None] * nb
            noise_stages = None
            if self.image_noise_mode:
                noise_stages = torch.empty(nb, dtype=i32, device=dev)
                noise_params = torch.empty((nb, 5), dtype=torch.float64, device=dev)
                batch_local32, batch_split = meta[2 * n + nb:], self._split_index.index_select(0, batch_frames)
            cam_p = self._cam_p.index_select(0, batch_frames)
            groups = self._group_host[sorted_frames]
            k0 = 0
            while k0 < nb:
                k1 = k0
                while k1 < nb and groups[k1] == groups[k0]:
                    k1 += 1
                g = self._groups[groups[k0]]
                a, b = int(starts[k0]), int(starts[k1])
                if not self.is_test:
                    _lib.check(L.mpsr_instance_xyz_crops_status(
                        _lib.ptr(g.depth), _lib.ptr(g.inst), _lib.ptr(g.p2), len(g.frames), g.shape[0], g.shape[1],
                        _lib.ptr(slot_local[a:b]), _lib.ptr(instance_id[a:b]), _lib.ptr(rows['boxes_2d'][a:b]),
                        _lib.ptr(rows['boxes_3d'][a:b]), _lib.ptr(rows['est_view_angs'][a:b]), b - a, roi_h, roi_w,
                        instance_utils._CENTROID_TYPES[self.centroid_type], int(self.rotate_view),
                        _lib.ptr(local[a:b]), _lib.ptr(glob[a:b]), _lib.ptr(valid[a:b]), _lib.ptr(self._status),
                        stream))
                if self.image_noise_mode:
                    images = torch.empty((k1 - k0,) + g.shape + (3,), dtype=f32, device=dev)
                    _lib.check(L.mpsr_image_noise(
                        _lib.ptr(g.rgb), len(g.frames), g.shape[0], g.shape[1], _lib.ptr(batch_local32[k0:k1]),
                        _lib.ptr(batch_split[k0:k1]), k1 - k0, self.seed & 0xFFFFFFFFFFFFFFFF, int(epoch),
                        self.image_noise_mode, _lib.ptr(images), _lib.ptr(noise_stages[k0:k1]),
                        _lib.ptr(noise_params[k0:k1]), stream))
                else:
                    images = g.rgb.index_select(0, batch_local[k0:k1]).float()
                for k in range(k0, k1):
                    rgb[k] = images[k - k0]
                k0 = k1
        samples = [None] * nb
        for k in range(nb):
            a, b = int(starts[k]), int(starts[k + 1])
            frame = self._frames[sorted_frames[k]]
            sample = {key: t[a:b] for key, t in rows.items()}
            if self.is_test:
                sample.update(rgb_image=rgb[k], cam_p=cam_p[k], sample_name=frame['name'], num_objs=frame['num_objs'])
            else:
                sample.update(rgb_image=rgb[k], cam_p=cam_p[k], gt_inst_xyz_maps_local=local[a:b],
                              gt_inst_xyz_maps_global=glob[a:b], gt_valid_mask_maps=valid[a:b],
                              sample_name=frame['name'], num_objs=frame['num_objs'],
                              oversample_indices=over_idx[a:b], jitter_trials=trials[a:b])
                if noise_stages is not None:
                    sample['image_noise_stages'] = noise_stages[k]
            samples[order[k]] = sample
        return samples
