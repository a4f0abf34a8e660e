"""What tests/test_train_loop_gpu.py shares: a five-frame 'train' split written from tests/golden (the `root` fixture of
tests/test_kitti_dataset_gpu.py: fixture depth maps, instance images, labels and cameras, a seeded synthetic RGB), the
narrow two-trunk trainer, and the loop's settings."""
import os

import numpy as np
from PIL import Image

from monopsr_amd.core.config_utils import ConfigObj

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# name in the split -> fixture frame; 000000 holds one Pedestrian and keeps no label: four frames train
SPLIT = (('000000', '000000'), ('000006', '000006'), ('000001', '000001'), ('000010', '000006'), ('000002', '000002'))
FILTER = dict(difficulty_str='all', box_2d_height=None, truncation=None, occlusion=None, depth_range=[5, 80])
DIV, NUM_BOXES, FRAMES_PER_STEP = 8, 8, 2
LEARNING_RATE = 1e-4
NAME = 'monopsr'


def write_split(top):
    """-> dataset_dir `top` with train.txt and training/{label_2, calib, image_2, depth_2_multiscale,
    instance_2_depth_2_multiscale}."""
    fix = np.load(os.path.join(GOLDEN, 'instance_fixture.npz'))
    split = os.path.join(top, 'training')
    dirs = ('label_2', 'calib', 'image_2', 'depth_2_multiscale', 'instance_2_depth_2_multiscale')
    for d in dirs:
        os.makedirs(os.path.join(split, d))
    rng = np.random.default_rng(0)
    for name, f in SPLIT:
        depth = Image.open(os.path.join(GOLDEN, 'depth_%s.png' % f))
        with open(os.path.join(split, 'label_2', name + '.txt'), 'w') as out:
            out.write(str(fix['labels_%s' % f]))
        p2 = ' '.join('%.12e' % v for v in fix['p2_%s' % f].reshape(-1))
        with open(os.path.join(split, 'calib', name + '.txt'), 'w') as out:
            out.write('P2: %s\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\n' % p2)
        w, h = depth.size
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(
            os.path.join(split, 'image_2', name + '.png'))
        depth.save(os.path.join(split, dirs[3], name + '.png'))
        Image.open(os.path.join(GOLDEN, 'instance_%s.png' % f)).save(os.path.join(split, dirs[4], name + '.png'))
    with open(os.path.join(top, 'train.txt'), 'w') as out:
        out.write(''.join(name + '\n' for name, _ in SPLIT))
    return top


def dataset_config(root):
    return dict(name='kitti', dataset_dir=root, data_split='train', data_split_dir='training', num_boxes=NUM_BOXES,
                classes=['Car'], oversample=True, num_alpha_bins=12, alpha_bin_overlap=0.0, use_mscnn_detections=True,
                obj_filter_config=dict(FILTER), aug_config=dict(use_image_aug=False, box_jitter_type='oversample'),
                depth_version='multiscale', instance_version='depth_2_multiscale', batch_size=FRAMES_PER_STEP)


def train_config(max_iterations=6, checkpoint_interval=3, summary_interval=2, **over):
    """A constant learning rate, the moving average on (a resumed run must carry it over)."""
    cfg = dict(max_iterations=max_iterations, checkpoint_interval=checkpoint_interval,
               summary_interval=summary_interval,
               optimizer=dict(optimizer_type='adam_optimizer', adam_optimizer=dict(
                   learning_rate_type='constant_learning_rate', learning_rate=LEARNING_RATE, use_moving_average=True,
                   moving_average_decay=0.9999)))
    cfg.update(over)
    return cfg


def make_dataset(root, seed=0):
    from monopsr_amd.datasets.kitti import kitti_dataset
    return kitti_dataset.KittiDataset(ConfigObj(dataset_config(root)), 'train', seed=seed)


def make_trainer(seed=43):
    from monopsr_amd.core import config_utils, train_net, trainer
    from monopsr_amd.core import weights as W
    cfg = config_utils.default_config()
    net = train_net.TrainNet(W.synthetic_weights(seed=seed, width_div=DIV, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                             width_div=DIV, full_trunk=True)
    return trainer.InstanceTrainer(net, cfg.model_config, cfg.dataset_config, train_config=ConfigObj(train_config()))


def reset(tr, params0):
    """The trainer as it was built: the initial parameters, no optimizer state, step 0."""
    net = tr.net
    net.params.copy_(params0)
    net.adam_m.zero_()
    net.adam_v.zero_()
    net.step_count = 0
    tr.global_step = 0
    tr.optimizer.shadow = None


def steps_in(directory, name=NAME):
    """{step: sorted suffixes} of the `<name>-<step, 8 digits>.<suffix>` files of a directory."""
    out = {}
    for entry in os.listdir(directory):
        if entry.startswith(name + '-'):
            step, suffix = entry[len(name) + 1:].split('.', 1)
            out.setdefault(int(step), []).append(suffix)
    return {k: sorted(v) for k, v in out.items()}


def read_csv(path):
    """-> (header names, rows as lists of float) of train_log.csv; the line ends must be CRLF."""
    with open(path, 'rb') as f:
        text = f.read().decode('ascii')
    assert text.endswith('\r\n') and text.count('\n') == text.count('\r\n')
    lines = [[c.strip() for c in line.split(',')] for line in text.split('\r\n')[:-1]]
    return lines[0], [[float(c) for c in line] for line in lines[1:]]


def is_dtoh(name):  # (tests/test_kitti_dataset_gpu.py)
    n = name.lower().replace(' ', '').replace('_', '')
    return 'dtoh' in n or 'devicetohost' in n or 'device->host' in n or 'device->pageable' in n or 'device->pinned' in n
