"""pose_estimation_amd — MI355X-native KRRN dense-fusion inference path of
yaomy533/pose_estimation (HRNet + heads + 3D-GCN fusion + TBase + PnP-RANSAC), with every
arithmetic step in the gfx950 HIP library libkrrn_hip.so (include/krrn_hip.h).

Drop-in API (the reference's names):
    KRRN(num_cls, cfg)                    lib/network/krrn.py
    get_pose(pred, data)                  tools/trainer.py:383-438 (Trainer.get_pose)
    estimateSimilarityTransform(src, dst) lib/transform/umeyama.py:8-98 (Umeyama-RANSAC, batched)
    get_pose_umeyama(pred, data)          tools/script/eval.py:128,151 (the depth-based pose)
    refine_pose_icp(R, t, data, diameter) ICP polish against the depth cloud (icp.py; this project's own)
    refine_pose_depth(R, t, data, dataset, diameter)  render-based point-to-plane polish on the depth frame
                                          (depth_refine.py; this project's own)
    PoseDataset / make_batch              dataset/linemod/batchdataset.py (synthetic frames)
    Metric                                lib/utils/metric.py
    KRRNLoss                              lib/network/loss.py (eval-time terms)
    dataset.PoseDataset / BucketBatcher   dataset/linemod/batchdataset.py + trainer.py:521-551
    evaluate.test_epoch                   tools/trainer.py:145-250 (batched)
    fps.farthest_point_sampling           tools/script/sample_model.py:35-48
    bpnp.BPnP / bpnp.BPnPModle            lib/network/dnn/BPnP.py (forward LM + implicit backward)
    raster.render_maps / PoseDataset(gt_maps=True)  the GT xyz / normal / region maps, rendered (this project's own)
    bop.vsd / bop.mssd_mspd / test_epoch(bop=True)  the BOP-19 pose errors and average recalls (no reference counterpart)
    verify.score_poses / select_pose / test_epoch(select="depth")  pose candidates scored against the observed depth,
                                          the best kept (render-and-compare; this project's own)
    rle.decode / PoseDataset(detections=...)  crops and masks from BOP detection files, RLE masks decoded on the GPU
    rle.encode_planes / bop_scene.write_gt_coco / test_epoch(seg_json=...)  masks encoded to RLE on the GPU: COCO
                                          ground truth, and the estimates' masks as a detection file
    bop_scene.eval_coco / rle.iou / coco.match / test_epoch(seg_json=..., coco=True)  COCO AP of detection and
                                          segmentation result files, mask IoU from the run lists on the GPU
    scene.render / scene.overlay / bop_scene.vis_results / test_epoch(vis_dir=...)  all instances of a frame in one
                                          z-buffer, and the estimates drawn on their frames (this project's own)
    models.extent / models.symmetry_residual / bop_scene.write_models_info / check_models_info  model diameters and
                                          boxes (BOP's calc_model_info) and a check of the declared symmetries
    models.sample_surface / bop_scene.write_models_eval / PoseDataset(model_points="surface")  model points drawn
                                          uniformly on the mesh surface, then FPS (tools/script/sample_model.py:35-76)
"""
from .config import CONFIG, Cfg, make_config  # noqa: F401
from .krrn import KRRN  # noqa: F401
from . import bpnp, dataset, fps  # noqa: F401
from .loss import KRRNLoss  # noqa: F401
from . import bop, coco, depth_refine, icp, models, raster, rle, scene, verify  # noqa: F401
from .pose import (add_icp_ops, add_umeyama_ops, get_pose, get_pose_umeyama, refine_pose_depth,  # noqa: F401
                   refine_pose_icp, select_pose)
from .umeyama import estimateSimilarityTransform  # noqa: F401

__all__ = ["KRRN", "KRRNLoss", "get_pose", "get_pose_umeyama", "add_umeyama_ops", "estimateSimilarityTransform",
           "bop", "coco", "depth_refine", "icp", "models", "raster", "rle", "scene", "verify", "refine_pose_depth", "refine_pose_icp", "select_pose",
           "add_icp_ops", "make_config", "CONFIG", "Cfg"]
