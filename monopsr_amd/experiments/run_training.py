"""Trains the instance path from a config on a KITTI split resident on the GPU (the reference's
experiments/run_training.py over core/trainer.py's loop; one process, one GPU).

    python -m monopsr_amd.experiments.run_training CONFIG --output-dir DIR
        [--data-split train] [--frames-per-step N]
        [--pretrained CKPT | --init-checkpoint CKPT | --synthetic-weights SEED]
        [--width-div N] [--seed S] [--image-noise reference|composed] [--decoder-bn frozen|batch]
        [--on-nonfinite stop|continue]

Under DIR: <config name>.yaml (a copy of CONFIG), train_state/ (what a later run of the same command resumes from),
checkpoints/ (what `python -m monopsr_amd.experiments.run_evaluation CONFIG --checkpoint-dir DIR/checkpoints --repeat ...`
scores in a second process while this one trains) and logs/train/train_log.csv.  core/train_loop.py has the details.
"""
import argparse
import datetime
import filecmp
import os
import shutil
import sys

WEIGHT_OPTIONS = ('--pretrained', '--init-checkpoint', '--synthetic-weights')


def build_parser():
    ap = argparse.ArgumentParser(description='train the instance path from a config')
    ap.add_argument('config', help='experiment config (yaml)')
    ap.add_argument('--output-dir', required=True, help='where the config copy, checkpoints and logs go')
    ap.add_argument('--data-split', default='train')
    ap.add_argument('--frames-per-step', type=int, default=None,
                    help='frames per training step (default: dataset_config.batch_size, or 1)')
    init = ap.add_mutually_exclusive_group()
    init.add_argument('--pretrained', metavar='CKPT',
                      help='Object-Detection-API checkpoint: its one ResNet-101 initialises both trunks')
    init.add_argument('--init-checkpoint', metavar='CKPT', help='a full checkpoint of the instance path')
    init.add_argument('--synthetic-weights', metavar='SEED', type=int, help='seeded random weights (dry runs, tests)')
    ap.add_argument('--width-div', type=int, default=1, help='channel divisor of the net (narrow nets for dry runs)')
    ap.add_argument('--seed', type=int, default=0, help="seed of the dataset's shuffling, jitter and image noise")
    ap.add_argument('--image-noise', choices=('reference', 'composed'), default=None,
                    help='which image noise aug_config.use_image_aug applies (KittiDataset)')
    ap.add_argument('--decoder-bn', choices=('frozen', 'batch'), default='frozen')
    ap.add_argument('--on-nonfinite', choices=('stop', 'continue'), default='stop')
    return ap


def config_name(cfg, config_path):
    return cfg.get('config_name') or os.path.splitext(os.path.basename(config_path))[0]


def copy_config(config_path, output_dir, name, now=None):
    """The reference's rule (experiments/run_training.py:52-66): copy the config to <output_dir>/<name>.yaml; when a copy
    is there and differs, keep it as <copy>.<str(datetime.now())> and replace it.  -> (copy path, backup path or None)."""
    os.makedirs(output_dir, exist_ok=True)
    copy_path = os.path.join(output_dir, '{}.yaml'.format(name))
    backup_path = None
    if os.path.exists(copy_path) and not filecmp.cmp(config_path, copy_path, shallow=False):
        datetime_str = str(now if now is not None else datetime.datetime.now())
        backup_path = copy_path + '.' + datetime_str
        shutil.copyfile(copy_path, backup_path)
        print('Config file has changed since ', datetime_str)
    if backup_path is not None or not os.path.exists(copy_path):
        shutil.copyfile(config_path, copy_path)
    return copy_path, backup_path


def will_resume(train_config, output_dir):
    """Whether core/train_loop.train will restore a checkpoint of <output_dir>/train_state."""
    overwrite = bool(getattr(train_config, 'overwrite_checkpoints', False)) if train_config is not None else False
    return not overwrite and os.path.exists(os.path.join(output_dir, 'train_state', 'checkpoint'))


def initial_weights(args, resume):
    """The variable dict the net is built from.  Nothing to resume and none of WEIGHT_OPTIONS: SystemExit."""
    given = [o for o, v in zip(WEIGHT_OPTIONS, (args.pretrained, args.init_checkpoint, args.synthetic_weights))
             if v is not None]
    if not given and not resume:
        raise SystemExit('nothing to resume in %s: give one of %s' % (os.path.join(args.output_dir, 'train_state'),
                                                                      ', '.join(WEIGHT_OPTIONS)))
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    seed = args.synthetic_weights if args.synthetic_weights is not None else 0
    weights = W.synthetic_weights(seed=seed, width_div=args.width_div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE))
    if args.pretrained is not None:
        restored = checkpoint_utils.restore_obj_detection_api_weights(
            weights, checkpoint_utils.load_checkpoint(args.pretrained))
        print('{} variables restored from {}'.format(len(restored), args.pretrained))
    elif args.init_checkpoint is not None:
        restored = checkpoint_utils.restore_monopsr_weights(weights,
                                                            checkpoint_utils.load_checkpoint(args.init_checkpoint))
        print('{} variables restored from {}'.format(len(restored), args.init_checkpoint))
    return weights


def main(argv=None):
    args = build_parser().parse_args(argv)
    from monopsr_amd.core import config_utils
    cfg = config_utils.parse_yaml_config(args.config)
    train_config = cfg.get('train_config')
    if train_config is None or getattr(train_config, 'max_iterations', None) is None:
        raise SystemExit('%s: train_config.max_iterations is missing' % args.config)
    weights = initial_weights(args, will_resume(train_config, args.output_dir))
    name = config_name(cfg, args.config)
    copy_config(args.config, args.output_dir, name)

    from monopsr_amd.core import train_loop, train_net, trainer
    from monopsr_amd.datasets.kitti.kitti_dataset import KittiDataset
    dataset_config, model_config = cfg.dataset_config, cfg.model_config
    dataset_config.data_split = args.data_split
    dataset = KittiDataset(dataset_config, 'train', seed=args.seed, image_noise=args.image_noise,
                           map_roi_size=tuple(getattr(model_config, 'map_roi_size', (48, 48))),
                           centroid_type=getattr(model_config, 'centroid_type', None),
                           rotate_view=getattr(model_config, 'rotate_view', True))
    net = train_net.TrainNet(weights, device=dataset.device, width_div=args.width_div, full_trunk=True,
                             decoder_bn=args.decoder_bn)
    tr = trainer.InstanceTrainer(net, model_config, dataset_config, train_config=train_config,
                                 classes_name=dataset.classes[0])
    frames_per_step = args.frames_per_step or int(getattr(dataset_config, 'batch_size', None) or 1)
    train_loop.train(tr, dataset, train_config, args.output_dir, frames_per_step=frames_per_step, name=name,
                     width_div=args.width_div, on_nonfinite=args.on_nonfinite)
    dataset.check_status()
    return 0


if __name__ == '__main__':
    sys.exit(main())
