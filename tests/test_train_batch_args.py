"""CPU checks of the multi-frame training step's boundary: the C ABI keeps its version and gains the five per-box-camera /
per-instance-scale entry points, and MonoPSRModel.build_train_batch refuses bad arguments before anything touches the GPU
(a model without a device net, samples on the CPU: reaching a launch would fail in another way)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monopsr_hip.h")
NEW = ("mpsr_proj_err_norm_cams", "mpsr_proj_err_norm_grad_cams", "mpsr_depth_map_local_to_global_cams",
       "mpsr_depth_map_local_to_global_grad_cams", "mpsr_huber_loss_grad_scales")


def _declared():  # (the parse of tests/test_cabi.py)
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mpsr_[a-z0-9_]+)\s*\(", text)))


def test_abi_version_stays_and_the_new_entry_points_are_declared():
    from monopsr_amd import _lib
    assert _lib.ABI_VERSION == 13
    declared = _declared()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert name in declared, name
    # camera entries: (n_cams, cam_index) follow cam_p; the scales entry has mpsr_huber_loss_grad's argument list
    assert _lib.SIGNATURES["mpsr_huber_loss_grad_scales"] == _lib.SIGNATURES["mpsr_huber_loss_grad"]
    for old in ("mpsr_proj_err_norm", "mpsr_proj_err_norm_grad", "mpsr_depth_map_local_to_global",
                "mpsr_depth_map_local_to_global_grad"):
        assert len(_lib.SIGNATURES[old + "_cams"][1]) == len(_lib.SIGNATURES[old][1]) + 2


def _frame(n=2, route="rgb_image"):
    z = lambda *s: torch.zeros(s)
    f = dict(boxes_2d=z(n, 4), cam_p=z(3, 4), est_view_angs=z(n), class_indices=torch.ones((n, 1), dtype=torch.int32),
             mean_lwh=z(n, 3), prop_cen_z_offset=z(n), boxes_3d=z(n, 7), gt_alpha_bins=torch.zeros(n, dtype=torch.int64),
             gt_alpha_regs=z(n, 12), gt_alpha_valid_bins=z(n, 12), gt_view_angs=z(n),
             gt_inst_xyz_maps_local=z(n, 48, 48, 3), gt_inst_xyz_maps_global=z(n, 48, 48, 3),
             gt_valid_mask_maps=z(n, 48, 48, 1))
    if route == "rgb_image":
        f.update(rgb_image=z(20, 30, 3), boxes_2d_norm=z(n, 4))
    else:
        f.update(rgb_image_crops=z(n, 48, 48, 3), full_img_feature_crop=z(n, 12, 12, 1024))
    return f


def _model(mode="train", fused=False):
    from monopsr_amd.core import config_utils
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    cfg = config_utils.default_config()
    return MonoPSRModel(cfg.model_config, cfg.dataset_config, None, mode, "Car", fused_heads=fused)


def test_build_train_batch_refuses_bad_arguments_before_any_launch():
    m = _model()
    with pytest.raises(ValueError, match="non-empty"):
        m.build_train_batch([])
    with pytest.raises(ValueError, match="frame 1 has no boxes"):
        m.build_train_batch([_frame(2), _frame(0)])
    with pytest.raises(ValueError, match="mixed input routes"):
        m.build_train_batch([_frame(2), _frame(3, "rgb_image_crops")])
    for key in ("gt_valid_mask_maps", "boxes_3d", "gt_alpha_valid_bins"):
        bad = _frame(2)
        del bad[key]
        with pytest.raises(ValueError, match=key):
            m.build_train_batch([_frame(1), bad])
    for mode, fused in (("test", True), ("test", False), ("train", True)):
        with pytest.raises(ValueError, match="built for training"):
            _model(mode, fused).build_train_batch([_frame(2)])


def test_step_batch_checks_its_arguments_first():
    """InstanceTrainer.step_batch validates before it zeroes the gradients (a trainer needs a net: checked on the
    model's own validator, the first thing step_batch calls)."""
    m = _model()
    route, counts = m._check_train_batch([_frame(2), _frame(5), _frame(1)])
    assert route == "rgb_image" and counts == [2, 5, 1]
