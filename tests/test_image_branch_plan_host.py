"""Which kernel runs each conv of the image branch (HRNet, the heads) is decided by shape eligibility
alone (hrnet._Builder.conv, runtime.add_gemm / conv_splits): the number of launches per entry point, over
every op whose name contains `conv` or `wino`, is pinned here at the BASELINE configurations' shapes.
Checked on CPU builds of the plan. The Winograd kernels take convs with >= 32768 output pixels, so the
B = 2 plans hold F(4x4) launches only at the large crops and no F(2x2) one; two shapes are built at
B = 64 as well, where both forms and the fused head run. The table was recorded from the tree before the
per-kernel environment switches were removed: a change of the dispatch moves it."""
import collections

import pytest
import torch

from pose_estimation_amd import KRRN, make_config
from pose_estimation_amd.krrn import KRRNPlan
from pose_estimation_amd.synthetic import init_weights

# (backbone, classes, S, N, B) -> launches per entry point
LAUNCHES = {
    ("lm", 1, 120, 1000, 2): {
        "krrn_conv1x1_nchw_f32": 1, "krrn_conv1x1_nchw_x3_f32": 1, "krrn_conv2d_f32": 51, "krrn_conv2d_x3_f32": 4,
        "krrn_convT_s2_x3_f32": 2, "krrn_conv_small_f32": 212, "krrn_gcn_conv_f32": 11},
    ("w18", 1, 120, 1000, 2): {
        "krrn_conv1x1_nchw_f32": 1, "krrn_conv1x1_nchw_x3_f32": 1, "krrn_conv2d_f32": 13, "krrn_conv2d_x3_f32": 3,
        "krrn_convT_s2_x3_f32": 2, "krrn_conv_small_f32": 299, "krrn_gcn_conv_f32": 11},
    ("w18", 13, 64, 1000, 2): {
        "krrn_conv1x1_nchw_f32": 1, "krrn_conv2d_f32": 10, "krrn_conv2d_x3_f32": 3, "krrn_convT_s2_x3_f32": 2,
        "krrn_conv_small_f32": 303, "krrn_gcn_conv_f32": 11},
    ("w18", 13, 200, 1000, 2): {
        "krrn_conv1x1_nchw_f32": 1, "krrn_conv2d_f32": 16, "krrn_conv2d_x3_f32": 7, "krrn_conv3x3_wino4_x3_f32": 3,
        "krrn_convT_s2_x3_f32": 2, "krrn_conv_small_f32": 290, "krrn_gcn_conv_f32": 11},
    ("w18", 5, 256, 1000, 2): {
        "krrn_conv1x1_nchw_f32": 1, "krrn_conv2d_f32": 15, "krrn_conv2d_x3_f32": 3, "krrn_conv3x3_wino4_x3_f32": 8,
        "krrn_convT_s2_x3_f32": 2, "krrn_conv_small_f32": 290, "krrn_gcn_conv_f32": 11},
    ("w32", 1, 320, 4096, 2): {
        "krrn_conv1x1_nchw_x3_f32": 1, "krrn_conv2d_f32": 52, "krrn_conv2d_x3_f32": 3, "krrn_conv3x3_wino4_x3_f32": 7,
        "krrn_conv3x3_wino4_x3_head_f32": 1, "krrn_convT_s2_x3_f32": 2, "krrn_conv_small_f32": 252,
        "krrn_gcn_conv_f32": 11},
    ("w18", 1, 64, 256, 2): {
        "krrn_conv1x1_nchw_f32": 1, "krrn_conv1x1_nchw_x3_f32": 1, "krrn_conv2d_f32": 9, "krrn_conv2d_x3_f32": 3,
        "krrn_convT_s2_x3_f32": 2, "krrn_conv_small_f32": 303, "krrn_gcn_conv_f32": 11},
    ("w18", 1, 120, 1000, 64): {
        "krrn_conv1x1_nchw_x3_f32": 1, "krrn_conv2d_f32": 6, "krrn_conv2d_x3_f32": 6, "krrn_conv3x3_wino4_x3_f32": 7,
        "krrn_conv3x3_wino4_x3_head_f32": 1, "krrn_conv3x3_wino_x3_f32": 5, "krrn_convT_s2_x3_f32": 2,
        "krrn_conv_small_f32": 284, "krrn_gcn_conv_f32": 20},
    ("lm", 1, 120, 1000, 64): {
        "krrn_conv1x1_nchw_x3_f32": 1, "krrn_conv2d_f32": 49, "krrn_conv2d_x3_f32": 25, "krrn_conv3x3_wino4_x3_f32": 7,
        "krrn_conv3x3_wino4_x3_head_f32": 1, "krrn_conv3x3_wino_x3_f32": 56, "krrn_convT_s2_x3_f32": 2,
        "krrn_conv_small_f32": 123, "krrn_gcn_conv_f32": 20},
}


@pytest.mark.parametrize("backbone,C,S,N,B", list(LAUNCHES))
def test_image_branch_convs_run_on_the_recorded_kernels(backbone, C, S, N, B):
    torch.manual_seed(0)
    m = KRRN(cfg=make_config(num_cls=C, backbone=backbone))
    init_weights(m, 0)
    m.eval()
    ops = KRRNPlan(m, B, S, N, True, torch.device("cpu")).plan.kernels()
    got = collections.Counter(op.name for op in ops if "conv" in op.name or "wino" in op.name)
    assert dict(got) == LAUNCHES[(backbone, C, S, N, B)]
    assert not [op.name for op in ops if op.name == "krrn_conv3x3_wino_f32"]
