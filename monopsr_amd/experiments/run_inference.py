"""Runs one checkpoint over a split of MSCNN 2-D detections in 'test' mode and writes what it predicts: the KITTI label
files and, per frame, the reconstructed scene (the reference's experiments/run_inference.py; the scenes are
core/scene_reconstruction.py).

    python -m monopsr_amd.experiments.run_inference CONFIG CHECKPOINT --mscnn-dir DIR --output-dir DIR
        [--data-split val|test] [--width-div N] [--no-scenes] [--min-score S] [--visible-only]
        [--surfaces [--max-edge-dz M] [--max-span-px N]] [--meshes [--mesh-visible-only]]

Under --output-dir: kitti_predictions_3d/<split>/<threshold>/<step>/data/<name>.txt as run_evaluation writes them, and
scenes/<split>/<step>/points/<name>.ply, depth/<name>.png, instances/<name>.png.  One network pass serves both: the
scenes are written from the Evaluator's chunks through its chunk_hook.  With --surfaces the instance maps are also
rendered as surfaces: depth_surface/<name>.png and instances_surface/<name>.png beside the three,
in the formats of depth/ and instances/.  With --meshes (which implies --surfaces) the drawn triangles are also written as
a coloured mesh per frame, mesh/<name>.ply with faces.  Split 'test' reads <dataset_dir>/testing and has
no labels; any other split reads the config's data_split_dir, and the AP report is printed when it has a label_2.
"""
import argparse
import os
import sys

from monopsr_amd.core import evaluator, scene_reconstruction


def build_parser():
    ap = argparse.ArgumentParser(description='KITTI label files and reconstructed scenes of one checkpoint on a split')
    ap.add_argument('config', help='experiment config (yaml)')
    ap.add_argument('checkpoint', help='checkpoint prefix, directory or .npz')
    ap.add_argument('--mscnn-dir', required=True, help='MSCNN detections in KITTI label format, one file per frame')
    ap.add_argument('--output-dir', required=True, help='where the label files and the scenes are written')
    ap.add_argument('--data-split', default='val', help="'test' reads <dataset_dir>/testing and has no labels")
    ap.add_argument('--width-div', type=int, default=1, help='channel divisor of the net the checkpoint was saved from')
    ap.add_argument('--no-scenes', action='store_true', help='write the label files only')
    ap.add_argument('--min-score', type=float, default=None,
                    help='2-D detection score a box needs to enter the scene (default: the label files\' threshold)')
    ap.add_argument('--visible-only', action='store_true',
                    help='keep only the points that win their pixel (drop what another point hides)')
    ap.add_argument('--surfaces', action='store_true',
                    help='also render the instance maps as surfaces: depth_surface/ and instances_surface/')
    ap.add_argument('--max-edge-dz', type=float, default=scene_reconstruction.SURFACE_MAX_EDGE_DZ,
                    help='--surfaces: a triangle whose depths span more than this many metres is not drawn')
    ap.add_argument('--max-span-px', type=int, default=scene_reconstruction.SURFACE_MAX_SPAN_PX,
                    help='--surfaces: nor is a triangle that spans more than this many pixels')
    ap.add_argument('--meshes', action='store_true',
                    help='also write the surfaces as coloured meshes, mesh/<name>.ply with faces (implies --surfaces)')
    ap.add_argument('--mesh-visible-only', action='store_true',
                    help='--meshes: only the triangles that win at least one pixel (drop what another surface hides)')
    ap.add_argument('--fit-centroids', action='store_true',
                    help='fit every predicted centroid to its 2-D box first: labels and scenes hold the fitted boxes')
    ap.add_argument('--fit-viewing-angle', action='store_true',
                    help='--fit-centroids: fit the viewing angle as well')
    return ap


def scene_dir(output_dir, data_split, global_step):
    return os.path.join(output_dir, 'scenes', data_split, str(global_step))


class SceneWriter(object):
    """An Evaluator chunk_hook: reconstruct_frames of every chunk, save_frame of every frame.  `base` is the directory
    that takes points/, depth/ and instances/; names collects the frames written.  surfaces: None, or the dict of
    options reconstruct_frames takes: depth_surface/ and instances_surface/ are written as well, and with 'mesh' in it
    mesh/."""

    def __init__(self, model, base, min_score=None, visible_only=False, surfaces=None):
        self.model, self.base, self.min_score, self.visible_only = model, base, min_score, bool(visible_only)
        self.surfaces = surfaces
        self.meshes = bool(surfaces and surfaces.get('mesh'))
        self.names = []
        self._dirs = self._surface_dirs = self._mesh_dirs = None

    def _make_dirs(self):
        if self._dirs is None:
            self._dirs = scene_reconstruction.scene_output_dirs(self.base)
            if self.surfaces is not None:
                self._surface_dirs = scene_reconstruction.surface_output_dirs(self.base)
            if self.meshes:
                self._mesh_dirs = scene_reconstruction.mesh_output_dirs(self.base)

    def __call__(self, rows, samples, outs):
        self._make_dirs()
        scene = scene_reconstruction.reconstruct_frames(self.model, samples, outs, self.min_score, self.visible_only,
                                                        surfaces=self.surfaces)
        for f, s in enumerate(samples):
            scene_reconstruction.save_frame(self._dirs, s['sample_name'], scene.frame(f))
            if self.surfaces is not None:
                scene_reconstruction.save_surface_frame(self._surface_dirs, s['sample_name'], scene.surfaces.frame(f))
            if self.meshes:
                scene_reconstruction.save_mesh_frame(self._mesh_dirs, s['sample_name'], scene.meshes.frame(f))
            self.names.append(s['sample_name'])

    def finish(self, dataset):
        """The frames of the split that keep no detection are no sample of the dataset: an empty scene for each, as the
        Evaluator writes an empty label file for them."""
        from monopsr_amd.datasets.kitti import depth_map_utils
        self._make_dirs()
        done = set(self.names)
        for name in dataset.split_sample_names:
            if name not in done:
                shape = depth_map_utils.image_shape(os.path.join(dataset.rgb_image_dir, name + '.png'))
                scene_reconstruction.save_empty_frame(self._dirs, name, shape)
                if self.surfaces is not None:
                    scene_reconstruction.save_empty_surface_frame(self._surface_dirs, name, shape)
                if self.meshes:
                    scene_reconstruction.save_empty_mesh_frame(self._mesh_dirs, name)
                self.names.append(name)


def parse_args(ap, argv=None):
    """The parsed command line; --meshes implies --surfaces."""
    args = ap.parse_args(argv)
    if args.mesh_visible_only and not args.meshes:
        ap.error('--mesh-visible-only needs --meshes')
    args.surfaces = args.surfaces or args.meshes
    return args


def surface_options(args):
    """-> the `surfaces` of reconstruct_frames the command line asks for (None: no surfaces)."""
    if not args.surfaces:
        return None
    options = dict(max_edge_dz=args.max_edge_dz, max_span_px=args.max_span_px)
    if args.meshes:
        options.update(mesh=True, mesh_visible_only=args.mesh_visible_only)
    return options


def main(argv=None):
    ap = build_parser()
    args = parse_args(ap, argv)
    centroid_fit = evaluator.centroid_fit_options(ap, args)
    from monopsr_amd.core import config_utils
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    from monopsr_amd.datasets.kitti.kitti_dataset import KittiDataset
    cfg = config_utils.parse_yaml_config(args.config)
    dcfg = cfg.dataset_config
    dcfg.data_split = args.data_split
    dcfg.use_mscnn_detections = True
    if args.data_split == 'test':
        dcfg.data_split_dir = 'testing'
        dcfg.has_kitti_labels = False
    else:
        split_dir = os.path.join(os.path.expanduser(dcfg.dataset_dir), getattr(dcfg, 'data_split_dir', 'training'))
        dcfg.has_kitti_labels = os.path.isdir(os.path.join(split_dir, 'label_2'))
    dataset = KittiDataset(dcfg, 'test', mscnn_label_dir=args.mscnn_dir)
    model = MonoPSRModel(cfg.model_config, dcfg, None, 'test')
    threshold = getattr(cfg.get('train_config'), 'kitti_score_threshold', 0.1)
    ev = evaluator.Evaluator(model, dataset, score_threshold=threshold, predictions_base_dir=args.output_dir,
                             centroid_fit=centroid_fit)
    step = ev.restore_checkpoint(args.checkpoint, width_div=args.width_div)
    writer = None
    if not args.no_scenes:
        writer = SceneWriter(model, scene_dir(args.output_dir, dataset.data_split, step),
                             ev.score_threshold if args.min_score is None else args.min_score, args.visible_only,
                             surface_options(args))
        ev.chunk_hook = writer
    result = ev.run_once(step)
    if writer is not None:
        writer.finish(dataset)
    if result['report'] is not None:
        sys.stdout.write(result['report'])
    sys.stdout.write('%d detections in %d of %d frames: %s\n' % (
        result['num_detections'], result['num_frames_with_detections'], result['num_frames'],
        result['kitti_predictions_dir']))
    if writer is not None:
        sys.stdout.write('%d scenes: %s\n' % (len(writer.names), writer.base))
    if 'centroid_fit' in result:
        sys.stdout.write('centroid fit: %s\n' % evaluator.format_centroid_fit(result['centroid_fit']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
