"""Relative-position tables on 14x14 windows at head_dim 64 (experiments/imagenet/cvt_v4/res_stem/s1_rpe_w14.yaml), without a GPU:
the module tree builds, and the host-side composition of one training step -- kernels replaced by their torch restatement,
oracle/ops_ref.py -- reproduces the reference's own step (tests/golden/nano_cvt_rpe_w14.pt, tools/gen_cvt_rpe_w14_golden.py)."""
import os

import pytest
import torch

from oracle import ref_loader as RL
from tests import golden_utils as GU
from tests.test_composition_cpu import build_cvt_variant, check_nano_cvt, cpu_ops  # noqa: F401  (cpu_ops: fixture)
from tests.test_oracle_cpu import GOLD

FIXTURE = os.path.join(GOLD, "nano_cvt_rpe_w14.pt")


def load_fixture():
    g = torch.load(FIXTURE, weights_only=False)
    c = g["case"]
    assert c["cfg"]["windows"] == (14, 7) and c["cfg"]["rel_pos_embed"] and c["cfg"]["res_stem"] and c["cfg"]["dims"][0] // c["cfg"]["heads"][0] == 64
    return g


def nano_pair(case, dev="cpu"):
    student, teacher = build_cvt_variant(case), build_cvt_variant(case, teacher=True)
    GU.fill_state_dict(student.state_dict(), 0)
    GU.fill_state_dict(teacher.state_dict(), 7)
    for m in (student, teacher):
        for k, v in m.state_dict().items():
            if k.endswith("running_var"):
                v.abs_().add_(0.5)
    student.head.last_layer.weight_g.data.fill_(1)
    for p in teacher.parameters():
        p.requires_grad = False
    return student.to(dev), teacher.to(dev)


def run_step(case, student, teacher, loss_mod, dev="cpu"):
    crops = [c.to(dev) for c in GU.make_crops(case["B"], n_local=case["n_local"], sizes=case["sizes"])]
    loss_fn = loss_mod.DDINOLoss(GU.NANO_HEAD["out_dim"], 2 + case["n_local"], 0.04, 0.07, 5, 10).to(dev)
    t_out = teacher(crops[:2])
    s_out = student(crops)
    loss = loss_fn(s_out, t_out, 2, None)
    loss.backward()
    return s_out, t_out, loss


def test_nano_rpe_w14_constructs_with_the_reference_layout(lib_built):
    """(refused by the constructor before the head_dim-64 bias-gradient kernel existed)"""
    g = load_fixture()
    student = build_cvt_variant(g["case"])
    assert [(k, tuple(v.shape), str(v.dtype)) for k, v in student.state_dict().items()] == g["keys"]
    assert [n for n, _ in student.named_parameters()] == g["param_names"]
    tables = {n: tuple(p.shape) for n, p in student.named_parameters() if "rel_pos_bias_table" in n}
    assert sorted(tables.values()) == [(169, 2), (729, 1), (729, 1)] and sorted(tables) == sorted(g["table_grads"])


def test_full_s1_rpe_w14_spec_constructs(lib_built):
    """res_stem/s1_rpe_w14.yaml at full width: WINDOW_SIZE [14, 14, 14, 7], head_dim 64 in every stage, a table per attention"""
    from esvit_amd import config as CFG
    from esvit_amd import models
    for cfg in (RL.cvt_config(rel_pos_embed=True, res_stem=True, windows=(14, 14, 14, 7)),
                CFG.cvt_config("cvt_s1", REL_POS_EMBED=True, RES_STEM=True, WINDOW_SIZE=[14, 14, 14, 7])):
        m = models.build_model(cfg, is_teacher=True)
        tables = [tuple(p.shape) for n, p in m.named_parameters() if "rel_pos_bias_table" in n]
        assert tables == [(729, 1)] * 2 + [(729, 3)] * 2 + [(729, 6)] * 6 + [(169, 12)] * 2
    # a Swin block of the same shape (14x14 window, head_dim 64) builds as well
    swin = models.build_model(RL.swin_config(embed_dim=64, depths=(1, 1), heads=(1, 2), window=14), is_teacher=True)
    assert swin.layers[0].blocks[0].attn.relative_position_bias_table.shape == (729, 1)


def test_nano_rpe_w14_composition_matches_reference_golden(cpu_ops):  # noqa: F811
    """one step of the nano case on the torch restatement of every kernel: loss to 2e-5, every gradient norm to 2e-3 (the bounds of
    test_composition_cpu.py for the other CvT variants), the three table gradients element by element under the same relative bound"""
    import esvit_amd.loss as L
    g = load_fixture()
    student, teacher = nano_pair(g["case"])
    s_out, t_out, loss = run_step(g["case"], student, teacher, L)
    check_nano_cvt(g, student, s_out, t_out, loss, rt=3e-4, loss_tol=2e-5, grad_tol=2e-3, buf_tol=1e-4)
    got = dict(student.named_parameters())
    for n, ref in g["table_grads"].items():
        err = (got[n].grad - ref).abs().max().item()
        assert err <= 2e-3 * ref.abs().max().item(), (n, err, ref.abs().max().item())
