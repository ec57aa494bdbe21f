"""Swin-L (experiments/imagenet/swin/swin_large_patch4_window7_224.yaml: DIM_EMBED 192, heads 6-12-24-48, depths 2-2-18-2) at full
width: the case table of tests/golden/full_swin_large.pt (tools/gen_swin_large_golden.py; the contents per case of
tests/golden/full_configs.pt), the yaml's SPEC, and the step the CPU and GPU tests run against the fixture."""
import os

import torch

from tests import golden_utils as GU

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_swin_large.pt")
YAML = "experiments/imagenet/swin/swin_large_patch4_window7_224.yaml"
# MODEL.SPEC of the yaml, verbatim
SPEC = dict(PATCH_SIZE=4, DIM_EMBED=192, DEPTHS=[2, 2, 18, 2], NUM_HEADS=[6, 12, 24, 48], WINDOW_SIZE=7, MLP_RATIO=4, QKV_BIAS=True,
            DROP_RATE=0, ATTN_DROP_RATE=0, DROP_PATH_RATE=0.2, USE_APE=False, PATCH_NORM=True)
CASES = {
    "swin_l_w7_k8192_b2": dict(arch="swin_large_w7", yaml=YAML, K=8192, B=2, s_seed=51, t_seed=52, crop_seed=82),
}
CASE = "swin_l_w7_k8192_b2"
SAMPLE = GU.FULL_CFG_SAMPLE
# the widths the Swin-L step normalises: blocks, PatchMerging (4 C of the stage it leaves) and the final norm
LN_WIDTHS = (192, 384, 768, 1536, 3072)


def gold(name=CASE):
    return torch.load(GOLD, map_location="cpu", weights_only=False)[name]


def build_case(name, dev):
    """student / teacher / loss / crops of a CASES entry, as oracle.gen_golden._full_cfg_case builds them with the reference's modules"""
    import esvit_amd
    from esvit_amd import config as CFG
    c = CASES[name]
    K = c["K"]
    cfg = CFG.model_config(c["arch"], DROP_PATH_RATE=0.0)
    student = esvit_amd.build_model(cfg, use_dense_prediction=True)
    teacher = esvit_amd.build_model(cfg, is_teacher=True, use_dense_prediction=True)
    fea = student.num_features
    student.head, teacher.head = esvit_amd.DINOHead(fea, K), esvit_amd.DINOHead(fea, K)
    student.head_dense, teacher.head_dense = esvit_amd.DINOHead(fea, K), esvit_amd.DINOHead(fea, K)
    GU.fill_full_cfg_pair(student, teacher, c)
    student, teacher = student.to(dev), teacher.to(dev)
    loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.04, 0, 1).to(dev)
    crops = [x.to(dev) for x in GU.make_crops(c["B"], seed=c["crop_seed"])]
    return student, teacher, loss_fn, crops


def run_case(name, dev):
    """one forward / loss / backward -> (student, loss_fn, s_out, t_out, loss)"""
    student, teacher, loss_fn, crops = build_case(name, dev)
    with torch.no_grad():
        t_out = teacher(crops[:2])
    s_out = student(crops)
    loss = loss_fn(s_out, t_out, 0, None)
    loss.backward()
    loss_fn.synchronize()
    return student, loss_fn, s_out, t_out, loss


def deltas(g, student, s_out, loss_fn, loss):
    """-> dict(outputs_rel, abs_err (loss), worst_grad_norm_rel, worst_sampled_grad_rel_l2, worst_tensor, center_abs)"""
    from tests.test_step_gpu import full_case_deltas
    out_rel, norm_rel, worst, worst_name = full_case_deltas(g, student, s_out, SAMPLE)
    c_err = max((loss_fn.center.cpu() - g["center"]).abs().max().item(), (loss_fn.center_grid.cpu() - g["center_grid"]).abs().max().item())
    return dict(loss=loss.item(), ref=g["loss"], abs_err=abs(loss.item() - g["loss"]), outputs_rel=out_rel, center_abs=c_err,
                worst_grad_norm_rel=norm_rel, worst_sampled_grad_rel_l2=worst, worst_tensor=worst_name)


def check_layout(g, student, s_out):
    assert [k for k, _ in student.named_parameters()] == g["param_names"]
    assert [(k, tuple(v.shape)) for k, v in student.state_dict().items()] == g["keys"]
    assert list(s_out[3]) == g["npatch"]
