"""-m gpu: the whole EsViT step through the HIP path vs (a) the golden vectors generated from the reference
(nano Swin, all 14 window geometries of 224/96 crops) and (b) the CPU oracle on real Swin-T widths."""
import math
import os

import pytest
import torch

from oracle import esvit_oracle as O
from tests import golden_utils as GU
from tests.test_composition_cpu import (build_nano, check_drop_path_vs_oracle, check_nano14, check_nano_cvt, check_odd_batches_vs_oracle, check_ragged_equals_reference_schedule, nano_cvt_pair, nano_pair, run_nano14_step,
                                        run_nano_cvt_step, run_nano_step)
from tests.test_oracle_cpu import GOLD, probe_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nano():
    return torch.load(os.path.join(GOLD, "nano_step.pt"), weights_only=False)


def _setup(prec):
    import esvit_amd
    assert torch.cuda.is_available()
    esvit_amd.set_precision(prec)
    return torch.device("cuda:0")


def _to(crops, dev):
    return [c.to(dev) for c in crops]


def _teardown():
    import esvit_amd
    esvit_amd.set_precision("bf16")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nano_step_matches_reference_golden(nano, prec, lib_built):
    import esvit_amd.loss as L
    dev = _setup(prec)
    try:
        student, teacher = nano_pair()
        student, teacher = student.to(dev), teacher.to(dev)
        nano_dev = dict(nano)
        nano_dev["center0"], nano_dev["center_grid0"] = nano["center0"].to(dev), nano["center_grid0"].to(dev)
        crops = _to(GU.make_crops(2), dev)
        s_out, t_out, loss, loss_fn = run_nano_step(nano_dev, student, teacher, L, crops, dev=dev)
        fp = prec == "fp32"
        rt = 3e-4 if fp else 3e-2
        for nm, t in (("s_cls", s_out[0]), ("s_reg", s_out[1]), ("s_fea", s_out[2]), ("t_cls", t_out[0]), ("t_reg", t_out[1]),
                      ("t_fea", t_out[2])):
            probe_close(nm, t.float().cpu(), nano[nm], rtol=rt)
        assert (list(s_out[3]), list(t_out[3])) == nano["npatch"]
        # loss within 1e-3 of the reference (north_star); fp32 mode is far tighter
        assert abs(loss.item() - nano["ddino_loss"]) < (1e-4 if fp else NANO_BF16["nano_step"][0]), (loss.item(), nano["ddino_loss"])
        tol_c = 1e-6 if fp else 7.5e-4  # (bf16: 2.5e-4 observed)
        assert (loss_fn.center.cpu() - nano["center1"]).abs().max().item() < tol_c
        assert (loss_fn.center_grid.cpu() - nano["center_grid1"]).abs().max().item() < tol_c
        assert [n for n, p in student.named_parameters() if p.grad is None] == nano["no_grad"]
        worst = 0.0
        for n, p in student.named_parameters():
            if p.grad is not None:
                ref = nano["grad_norms"][n]
                worst = max(worst, abs(p.grad.norm().item() - ref) / (ref + 1e-12))
                if fp:
                    probe_close("grad " + n, p.grad.cpu(), nano["grads"][n], rtol=2e-3)
        if not fp:
            GU.record_parity(test="nano_step", prec="bf16", abs_err=abs(loss.item() - nano["ddino_loss"]), worst_grad_norm_rel=worst,
                             center_err=max((loss_fn.center.cpu() - nano["center1"]).abs().max().item(),
                                            (loss_fn.center_grid.cpu() - nano["center_grid1"]).abs().max().item()))
        assert worst < (2e-3 if fp else NANO_BF16["nano_step"][1]), worst
        if fp:
            with torch.no_grad():
                probe_close("last_attn", student.forward_selfattention(crops[0]).cpu(), nano["last_attn"], rtol=3e-4)
    finally:
        _teardown()


def test_nano_fused_update_matches_reference_golden(nano, lib_built):
    """clip 3.0 -> AdamW -> EMA on the reference's own gradients (fp32 mode so that gradients agree to 1e-3)."""
    import esvit_amd.loss as L
    from esvit_amd.update import FusedClipAdamWEMA
    dev = _setup("fp32")
    try:
        student, teacher = nano_pair()
        student, teacher = student.to(dev), teacher.to(dev)
        nano_dev = dict(nano)
        nano_dev["center0"], nano_dev["center_grid0"] = nano["center0"].to(dev), nano["center_grid0"].to(dev)
        run_nano_step(nano_dev, student, teacher, L, _to(GU.make_crops(2), dev), dev=dev)
        upd = FusedClipAdamWEMA(student, teacher)
        assert [len(g["params"]) for g in upd.param_groups] == nano["group_sizes"]
        upd.step(5e-4, 0.04, 0.996, clip_grad=3.0)
        torch.cuda.synchronize()
        for n, p in student.named_parameters():
            probe_close("student_after " + n, p.detach().cpu(), nano["student_after"][n], rtol=2e-4)
        for n, p in teacher.named_parameters():
            probe_close("teacher_after " + n, p.detach().cpu(), nano["teacher_after"][n], rtol=2e-4)
    finally:
        _teardown()


@pytest.mark.parametrize("window", [7, 14])
def test_odd_batches_match_oracle_gpu(window, lib_built):
    """B = 1 and B = 3 through the HIP path (fp32 precision mode), 7x7 and 14x14 windows, vs the CPU oracle"""
    import esvit_amd.loss as L
    dev = _setup("fp32")
    try:
        check_odd_batches_vs_oracle(L, dev, window=window, tol=5e-4, gtol=1e-2)
    finally:
        _teardown()


def test_drop_path_matches_oracle_gpu(lib_built):
    """stochastic depth through the HIP path (fp32 precision mode) with fixed keep factors vs the CPU oracle"""
    import esvit_amd.loss as L
    dev = _setup("fp32")
    try:
        check_drop_path_vs_oracle(L, dev, tol=5e-4, gtol=1e-2)
    finally:
        _teardown()


def test_ragged_multi_crop_equals_reference_schedule_gpu(lib_built):
    """HIP path, fp32: ragged patch embedding / blocks / patch merging / final norm vs one pass per resolution group"""
    import esvit_amd.loss as L
    dev = _setup("fp32")
    try:
        check_ragged_equals_reference_schedule(L, dev, tol=2e-5)
    finally:
        _teardown()


FULL_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_width.pt")


def build_full_case(name, dev):
    """student / teacher / loss / crops of a tests/golden_utils.FULL_CASES entry, exactly as oracle/gen_golden.py:gen_full built
    them with the reference's modules (same seeds)"""
    import esvit_amd
    from esvit_amd import config as CFG
    c = GU.FULL_CASES[name]
    K, B = c["K"], c["B"]
    cfg = CFG.swin_config("swin_tiny_w7", DROP_PATH_RATE=0.0)
    student = esvit_amd.build_model(cfg, use_dense_prediction=c["dense"])
    teacher = esvit_amd.build_model(cfg, is_teacher=True, use_dense_prediction=c["dense"])
    student.head, teacher.head = esvit_amd.DINOHead(student.num_features, K), esvit_amd.DINOHead(teacher.num_features, K)
    if c["dense"]:
        student.head_dense = esvit_amd.DINOHead(student.num_features, K, norm_last_layer=(name != "swin_t_k8192_b2"))
        teacher.head_dense = esvit_amd.DINOHead(teacher.num_features, K)
    GU.fill_state_dict(student.state_dict(), c["s_seed"])
    GU.fill_state_dict(teacher.state_dict(), c["t_seed"])
    student.head.last_layer.weight_g.data.fill_(1)
    if c["dense"] and name == "swin_t_k65536_b8":
        student.head_dense.last_layer.weight_g.data.fill_(1)
    student, teacher = student.to(dev), teacher.to(dev)
    for p in teacher.parameters():
        p.requires_grad = False
    loss_fn = (esvit_amd.DDINOLoss(K, 10, 0.04, 0.04, 0, 1) if c["dense"] else esvit_amd.DINOLoss(K, 2, 0.04, 0.04, 0, 1)).to(dev)
    crops = [x.to(dev) for x in GU.make_crops(B, seed=c["crop_seed"])[:c["ncrops"]]]
    return student, teacher, loss_fn, crops


def run_full_case(name, dev, armed=False):
    """one forward / loss / backward of the case on the HIP path -> (student, loss_fn, s_out, t_out, loss).
    armed: the loss announces itself to the heads first, as engine.EsvitTrainer.step does (loss.arm_logit_stats)"""
    student, teacher, loss_fn, crops = build_full_case(name, dev)
    if armed:
        loss_fn.arm_logit_stats(student, teacher, 0)
    with torch.no_grad():
        t_out = teacher(crops[:2])
    s_out = student(crops)
    if armed:
        loss_fn.disarm_logit_stats(student, teacher)
    loss = loss_fn(s_out, t_out, 0, None)
    loss.backward()
    loss_fn.synchronize()
    return student, loss_fn, s_out, t_out, loss


def full_case_deltas(g, student, s_out, n=GU.FULL_SAMPLE):
    """-> (worst relative error of the sampled student outputs, worst relative gradient-norm error, worst relative L2 error of the
    sampled gradient tensors and its name).  Gradients that are ZERO in exact arithmetic are compared on an absolute scale: the
    LayerNorm weight in front of CvT's depthwise-conv + BatchNorm projection has no gradient (BatchNorm removes any per-channel
    scale), the reference's 1e-8 there is fp32 rounding noise -- denominators are floored at 1e-5 of the largest gradient norm."""
    outs = s_out[:3] if isinstance(s_out, (tuple, list)) else [s_out]
    out_rel = max(((GU.strided(o, n).float().cpu() - ref).abs().max() / mx).item() for o, ref, mx in zip(outs, g["s_out"], g["s_out_absmax"]))
    prm = dict(student.named_parameters())
    floor = 1e-5 * max(g["grad_norm"].values())
    norm_rel = max(abs(prm[k].grad.norm().item() - r) / max(r, floor) for k, r in g["grad_norm"].items())
    worst, worst_name = 0.0, ""
    for k, ref in g["sampled"].items():
        d = ((GU.strided(prm[k].grad, n).float().cpu() - ref).norm() / max(ref.norm().item(), floor)).item()
        if d > worst:
            worst, worst_name = d, k
    return out_rel, norm_rel, worst, worst_name


FULL_CFG_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_configs.pt")


def run_full_cfg_case(name, dev):
    """one forward / loss / backward of a tests/golden_utils.FULL_CFG_CASES entry (BASELINE configs 3-5 at full width) on the HIP
    path, built exactly as oracle/gen_golden.py:gen_full_configs built it with the reference's modules"""
    import esvit_amd
    from esvit_amd import config as CFG
    c = GU.FULL_CFG_CASES[name] if name in GU.FULL_CFG_CASES else GU.FULL_VIL_CASES[name]
    K, B = c["K"], c["B"]
    cfg = CFG.model_config(c["arch"], DROP_PATH=0.0) if c["arch"].startswith("vil_") else CFG.model_config(c["arch"], DROP_PATH_RATE=0.0)
    student = esvit_amd.build_model(cfg, use_dense_prediction=True)
    teacher = esvit_amd.build_model(cfg, is_teacher=True, use_dense_prediction=True)
    fea = student.num_features
    student.head, teacher.head = esvit_amd.DINOHead(fea, K), esvit_amd.DINOHead(fea, K)
    student.head_dense, teacher.head_dense = esvit_amd.DINOHead(fea, K), esvit_amd.DINOHead(fea, K)
    GU.fill_full_cfg_pair(student, teacher, c)
    student, teacher = student.to(dev), teacher.to(dev)
    loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.04, 0, 1).to(dev)
    crops = [x.to(dev) for x in GU.make_crops(B, seed=c["crop_seed"])]
    with torch.no_grad():
        t_out = teacher(crops[:2])
    s_out = student(crops)
    loss = loss_fn(s_out, t_out, 0, None)
    loss.backward()
    loss_fn.synchronize()
    return student, loss_fn, s_out, t_out, loss


# bf16 bounds per case: <= 3x the deltas observed on MI355X (profiles/r03_parity_observed.jsonl): (outputs, loss, grad norms, sampled)
# (observed in round 3: W14-T 8.2e-3 / 6.2e-4 / 1.4e-2 / 8.5e-2, W14-B 1.1e-2 / 3.7e-4 / 1.0e-2 / 5.7e-2, CvT-13 7.8e-3 / 1.4e-4 / 3.9e-2 / 6.6e-2)
FULL_CFG_BF16_BOUNDS = {
    "swin_t_w14_k8192_b2": (2.5e-2, 1.9e-3, 4.3e-2, 0.25),
    "swin_b_w14_k8192_b2": (3.2e-2, 1.1e-3, 3.2e-2, 0.17),
    "cvt13_s1_k8192_b2": (2.4e-2, 4.2e-4, 0.12, 0.2),
}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GU.FULL_CFG_CASES))
def test_baseline_configs_3_to_5_full_width_match_reference_golden(name, prec, lib_built):
    """BASELINE.json configs 3-5 at FULL width -- Swin-T W=14, Swin-B W=14 (widths 128 .. 1024, depths 2-2-18-2), CvT-13
    (cvt_v4 s1.yaml) -- 2x224^2 + 8x96^2 crops, V+R heads, DDINOLoss, B = 2, out_dim 8192: outputs, loss, centres, every gradient
    norm and sampled gradient tensors against the step of the REFERENCE's own modules built from its own experiment yamls
    (tests/golden/full_configs.pt, oracle/gen_golden.py:gen_full_configs)"""
    g = torch.load(FULL_CFG_GOLD, map_location="cpu", weights_only=False)[name]
    dev = _setup(prec)
    try:
        student, loss_fn, s_out, t_out, loss = run_full_cfg_case(name, dev)
        fp = prec == "fp32"
        assert [k for k, _ in student.named_parameters()] == g["param_names"]
        assert [(k, tuple(v.shape)) for k, v in student.state_dict().items()] == g["keys"]
        assert list(s_out[3]) == g["npatch"]
        out_rel, norm_rel, worst, worst_name = full_case_deltas(g, student, s_out, GU.FULL_CFG_SAMPLE)
        c_err = max((loss_fn.center.cpu() - g["center"]).abs().max().item(), (loss_fn.center_grid.cpu() - g["center_grid"]).abs().max().item())
        GU.record_parity(test=name, prec=prec, loss=loss.item(), ref=g["loss"], abs_err=abs(loss.item() - g["loss"]), outputs_rel=out_rel,
                         center_abs=c_err, worst_grad_norm_rel=norm_rel, worst_sampled_grad_rel_l2=worst, worst_tensor=worst_name)
        b_out, b_loss, b_norm, b_samp = (1e-4, 1e-4, 5e-3, 5e-3) if fp else FULL_CFG_BF16_BOUNDS[name]
        assert out_rel < b_out, out_rel
        assert abs(loss.item() - g["loss"]) < b_loss, (loss.item(), g["loss"])
        assert norm_rel < b_norm, norm_rel
        assert worst < b_samp, (worst_name, worst)
        assert c_err < (1e-6 if fp else 2e-3), c_err
    finally:
        _teardown()


FULL_VIL_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_vil.pt")
# (outputs, loss, grad norms, sampled): bf16 bounds <= 3x the deltas observed on MI355X (profiles/r03_parity_observed.jsonl)
# (observed in round 3: outputs 7.8e-3, loss 8.9e-5, gradient norms 5.5e-3, sampled gradients 3.5e-2; fp32 mode: loss exact, outputs 1.6e-6)
# (vil_small, observed in round 4: outputs 8.7e-3, loss 1.5e-4, gradient norms 4.1e-3, sampled gradients 0.108 -- the 8192 x 256 last-layer
# direction tensor of the dense head, whose entries are ~1e-6; fp32 mode: loss exact, outputs 2.4e-6; profiles/r04_parity_observed.jsonl)
FULL_VIL_BF16_BOUNDS = {"vil_tiny_k8192_b2": (2.4e-2, 2.7e-4, 1.7e-2, 0.11), "vil_small_k8192_b2": (2.6e-2, 4.5e-4, 1.2e-2, 0.32)}


def check_full_vil_case(name, dev, fp, bounds, record=None):
    """Vision Longformer at full width (vil_tiny: sliding-chunk attention in stages 1-2, head_dim 48 in stage 1, full attention in
    stages 3-4): module tree, outputs, loss, centres, every gradient norm, sampled gradients and the forward_return_n_last_blocks hook
    against the step of the REFERENCE's own MsViT built from its yaml (tests/golden/full_vil.pt, oracle/gen_golden.py:gen_full_vil)"""
    from esvit_amd.models import vision_longformer as _vil
    old_mode = _vil.SAME_SIZE_RESAMPLING
    _vil.SAME_SIZE_RESAMPLING = "cpu"  # the fixture is the reference's CPU run (torch's CPU bicubic kernel resamples at the construction resolution)
    try:
        _check_full_vil_case(name, dev, fp, bounds, record)
    finally:
        _vil.SAME_SIZE_RESAMPLING = old_mode  # (later tests in the same process see the library's default again)


def _check_full_vil_case(name, dev, fp, bounds, record):
    g = torch.load(FULL_VIL_GOLD, map_location="cpu", weights_only=False)[name]
    student, loss_fn, s_out, t_out, loss = run_full_cfg_case(name, dev)
    assert [k for k, _ in student.named_parameters()] == g["param_names"]
    assert [(k, tuple(v.shape)) for k, v in student.state_dict().items()] == g["keys"]
    assert list(s_out[3]) == g["npatch"]
    out_rel, norm_rel, worst, worst_name = full_case_deltas(g, student, s_out, GU.FULL_CFG_SAMPLE)
    c_err = max((loss_fn.center.cpu() - g["center"]).abs().max().item(), (loss_fn.center_grid.cpu() - g["center_grid"]).abs().max().item())
    if record:
        GU.record_parity(test=name, prec=record, loss=loss.item(), ref=g["loss"], abs_err=abs(loss.item() - g["loss"]), outputs_rel=out_rel,
                         center_abs=c_err, worst_grad_norm_rel=norm_rel, worst_sampled_grad_rel_l2=worst, worst_tensor=worst_name)
    b_out, b_loss, b_norm, b_samp = bounds
    assert out_rel < b_out, out_rel
    assert abs(loss.item() - g["loss"]) < b_loss, (loss.item(), g["loss"])
    assert norm_rel < b_norm, norm_rel
    assert worst < b_samp, (worst_name, worst)
    assert c_err < (1e-6 if fp else 2e-3), c_err
    student.eval()
    with torch.no_grad():
        crop = GU.make_crops(GU.FULL_VIL_CASES[name]["B"], seed=GU.FULL_VIL_CASES[name]["crop_seed"])[2][:1].to(dev)
        lb = student.forward_return_n_last_blocks(crop, n=4, depth=[cf['n'] for cf in student.layer_cfgs])
    ref = g["last_blocks"]
    assert lb.shape == ref.shape and ((lb.float().cpu() - ref).abs().max() / ref.abs().max()).item() < (1e-4 if fp else 3e-2)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GU.FULL_VIL_CASES))
def test_vil_full_width_matches_reference_golden(name, prec, lib_built):
    dev = _setup(prec)
    try:
        fp = prec == "fp32"
        check_full_vil_case(name, dev, fp, (1e-4, 1e-4, 5e-3, 5e-3) if fp else FULL_VIL_BF16_BOUNDS[name], record=prec)
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_swin_tiny_step_matches_reference_golden(prec, lib_built):
    """real Swin-T widths (96..768, heads 3..24), K = 8192, B = 2, 2x224 + 8x96 crops: outputs, loss, every gradient norm and
    twelve sampled gradient tensors against the step of the REFERENCE's own modules on the same weights and crops
    (tests/golden/full_width.pt, oracle/gen_golden.py:gen_full)."""
    g = torch.load(FULL_GOLD, map_location="cpu", weights_only=False)["swin_t_k8192_b2"]
    dev = _setup(prec)
    try:
        student, loss_fn, s_out, t_out, loss = run_full_case("swin_t_k8192_b2", dev)
        fp = prec == "fp32"
        out_rel, norm_rel, worst, worst_name = full_case_deltas(g, student, s_out)
        assert list(s_out[3]) == g["npatch"]
        GU.record_parity(test="swin_tiny_k8192_b2", prec=prec, loss=loss.item(), ref=g["loss"], abs_err=abs(loss.item() - g["loss"]),
                         outputs_rel=out_rel, worst_grad_norm_rel=norm_rel, worst_sampled_grad_rel_l2=worst, worst_tensor=worst_name)
        # bf16: <= 3x observed (profiles/r03_parity_observed.jsonl: outputs 8.1e-3, loss 2.8e-4, gradient norms 1.3e-2, sampled 7.6e-2)
        assert out_rel < (1e-4 if fp else 2.5e-2), out_rel
        assert abs(loss.item() - g["loss"]) < (1e-4 if fp else 8.4e-4), (loss.item(), g["loss"])
        assert norm_rel < (5e-3 if fp else 3.9e-2), norm_rel
        assert worst < (5e-3 if fp else 0.23), (worst_name, worst)
        assert (loss_fn.center.cpu() - g["center"]).abs().max().item() < (1e-6 if fp else 6e-4)
        assert (loss_fn.center_grid.cpu() - g["center_grid"]).abs().max().item() < (1e-6 if fp else 6e-4)
    finally:
        _teardown()


# bf16 bounds of the nano-width steps: (|loss - reference|, worst relative gradient-norm error), <= 3x the deltas observed on the MI355X
# (profiles/r03_parity_observed.jsonl)
# observed: nano_step 7.5e-4 / 0.81 %, nano_w14_step 6.7e-4 / 2.1 %, nano_cvt_step 8.0e-4 / 1.3 %
NANO_BF16 = {"nano_step": (2.4e-3, 0.025), "nano_w14_step": (2e-3, 0.06), "nano_cvt_step": (2.4e-3, 0.04)}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nano_w14_step_matches_reference_golden(prec, lib_built):
    """14x14 windows through the blocked attention kernels (window_attn_big.hip) vs the reference golden"""
    import esvit_amd.loss as L
    g14 = torch.load(os.path.join(GOLD, "nano14_step.pt"), weights_only=False)
    dev = _setup(prec)
    try:
        student, teacher = nano_pair(window=14)
        student, teacher = student.to(dev), teacher.to(dev)
        s_out, t_out, loss = run_nano14_step(student, teacher, L, dev=dev)
        fp = prec == "fp32"
        if not fp:
            GU.record_parity(test="nano_w14_step", prec="bf16", abs_err=abs(loss.item() - g14["ddino_loss"]),
                             worst_grad_norm_rel=max(abs(p.grad.norm().item() - g14["grad_norms"][n]) / (g14["grad_norms"][n] + 1e-12)
                                                     for n, p in student.named_parameters() if p.grad is not None))
        check_nano14(g14, student, s_out, t_out, loss, rt=3e-4 if fp else 3e-2, loss_tol=1e-4 if fp else NANO_BF16["nano_w14_step"][0],
                     grad_tol=2e-3 if fp else NANO_BF16["nano_w14_step"][1], probes=fp)
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nano_cvt_step_matches_reference_golden(prec, lib_built):
    """CvT (BASELINE config 5) through the HIP path: ConvEmbed im2col + GEMM, depthwise 3x3 + BatchNorm kernels, head_dim-64 window
    attention (7x7, padded 12 -> 14, 6x6, 3x3), QuickGELU GEMM epilogues -- forward, loss, every gradient, BN running statistics"""
    import esvit_amd.loss as L
    g = torch.load(os.path.join(GOLD, "nano_cvt_step.pt"), weights_only=False)
    dev = _setup(prec)
    try:
        student, teacher = nano_cvt_pair(dev)
        s_out, t_out, loss = run_nano_cvt_step(student, teacher, L, dev=dev)
        fp = prec == "fp32"
        if fp:
            check_nano_cvt(g, student, s_out, t_out, loss, rt=5e-4, loss_tol=1e-4, grad_tol=3e-3, buf_tol=1e-4)
        else:
            got = {n: p.grad for n, p in student.named_parameters() if p.grad is not None}
            GU.record_parity(test="nano_cvt_step", prec="bf16", abs_err=abs(loss.item() - g["ddino_loss"]),
                             worst_grad_norm_rel=max(max(abs(got[n].norm().item() - ref) - 1e-6, 0.0) / (ref + 1e-12) for n, ref in g["grad_norms"].items()))
            assert abs(loss.item() - g["ddino_loss"]) < NANO_BF16["nano_cvt_step"][0], (loss.item(), g["ddino_loss"])
            assert sorted(got) == sorted(g["grad_norms"])
            for n, ref in g["grad_norms"].items():
                assert abs(got[n].norm().item() - ref) <= NANO_BF16["nano_cvt_step"][1] * ref + 1e-6, (n, got[n].norm().item(), ref)
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GU.NANO_CVT_VARIANTS))
def test_cvt_variants_step_matches_reference_golden(name, prec, lib_built):
    """the CvT variants of the other cvt_v4 yaml files through the HIP path: relative-position tables and the unrolled shift mask in
    the head_dim-64 window attention (table gradient included), the residual stem's convolutions"""
    import esvit_amd.loss as L
    from tests.test_composition_cpu import check_cvt_variant
    dev = _setup(prec)
    try:
        if prec == "fp32":
            check_cvt_variant(name, L, dev=dev, rt=5e-4, loss_tol=1e-4, grad_tol=3e-3, buf_tol=1e-4)
        else:
            # observed (profiles/r03_parity_observed.jsonl): loss 4e-5 .. 9.6e-4, gradient norms 1.2 .. 2.7 %
            check_cvt_variant(name, L, dev=dev, rt=6e-2, loss_tol=3e-3, grad_tol=0.08, buf_tol=2e-2, probes=False)
    finally:
        _teardown()


def test_nano_cvt_eval_matches_reference_golden(lib_built):
    """eval-mode BatchNorm + forward_return_n_last_blocks of the CvT through the HIP path (fp32 precision mode)"""
    g = torch.load(os.path.join(GOLD, "nano_cvt_step.pt"), weights_only=False)
    dev = _setup("fp32")
    try:
        student, _ = nano_cvt_pair(dev)
        student.eval()
        crops = _to(GU.make_crops(2, n_local=3, sizes=GU.NANO_CVT["sizes"]), dev)
        with torch.no_grad():
            cls, region = student.forward_features(crops[0])
            probe_close("eval cls", cls.cpu(), g["eval_cls"], rtol=5e-4)
            probe_close("eval region", region.cpu(), g["eval_region"], rtol=5e-4)
            feats = student.forward_return_n_last_blocks(crops[2], n=2, depth=list(GU.NANO_CVT["depths"]))
        assert torch.allclose(feats.cpu(), g["eval_last_blocks"], rtol=5e-4, atol=2e-5)
    finally:
        _teardown()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_reference_written_checkpoint_through_the_knn_consumers_gpu(prec, lib_built):
    """a checkpoint file written by the reference's utils.save_on_master, loaded and evaluated end to end on the HIP path
    (load_pretrained_weights -> extract_features -> knn_classifier) against the reference's own features and k-NN votes"""
    from tests.test_composition_cpu import check_ref_checkpoint
    dev = _setup(prec)
    try:
        if prec == "fp32":
            check_ref_checkpoint(dev, tol=5e-6, top_tol=1.0)
        else:  # bf16 activations move the features by 4e-3 (observed) and with them at most a few of the hundred votes
            check_ref_checkpoint(dev, tol=1.2e-2, top_tol=3.0)
    finally:
        _teardown()


def test_eval_knn_consumers_gpu(lib_built):
    """SURVEY.md 8f-1 on the HIP path: extract_features through the backbone kernels, knn_classifier through the fp32 MFMA GEMM,
    against the reference's golden top-1 / top-5 and the CPU oracle on a larger set"""
    from esvit_amd import eval as E
    from tests.test_composition_cpu import check_extract_features
    dev = _setup("fp32")
    try:
        check_extract_features(dev, tol=2e-5)
        gold = torch.load(os.path.join(GOLD, "knn.pt"), weights_only=False)
        for c, want in zip(GU.KNN_CASES, gold["top"]):
            xtr, ytr, xte, yte = GU.make_knn_set(c["seed"], noise=c["noise"])
            got = E.knn_classifier(xtr.to(dev), ytr.to(dev), xte.to(dev), yte.to(dev), c["k"], c["T"], num_classes=10)
            assert got == pytest.approx(want, abs=0.26), (c, got, want)  # one borderline neighbour of 400 may flip under MFMA summation order
        xtr, ytr, xte, yte = GU.make_knn_set(11, n_train=20000, n_test=3000, dim=384, classes=100, noise=6.0)
        want = O.knn_classifier(xtr, ytr, xte, yte, 20, 0.07, num_classes=100)
        got = E.knn_classifier(xtr.to(dev), ytr.to(dev), xte.to(dev), yte.to(dev), 20, 0.07, num_classes=100)
        assert got == pytest.approx(want, abs=0.1), (got, want)
    finally:
        _teardown()


def test_eval_linear_probe_gpu(lib_built):
    """SURVEY.md 8f-1, eval_linear.py on the HIP path: frozen-backbone features, the probe's linear layer on the fp32 MFMA GEMM
    (forward + fused weight / bias gradient), SGD, validation -- against the fixture from the reference's own loop"""
    from tests.test_composition_cpu import check_linear_probe
    dev = _setup("fp32")
    try:
        check_linear_probe(dev, tol=3e-4)
    finally:
        _teardown()


def test_logit_stats_handover_is_taken_and_falls_back(lib_built):
    """engine.EsvitTrainer arms the heads so that their last-layer GEMMs emit the softmax row statistics of the coming loss
    (esvit_gemm_desc::rowstat -> loss.py): (1) with every logits tensor in whole 128-row tiles the loss really takes them -- not one
    esvit_teacher_row_stats launch in the step, and the CE kernel is handed the student statistics; (2) a centre update between the
    forwards and the loss changes the token, the loss falls back to its own passes and equals the un-armed loss (nothing
    tested which path ran)"""
    import esvit_amd.loss as L
    from esvit_amd import engine, ops
    dev = _setup("bf16")
    calls = {"teacher_row_stats": 0, "ce_with_student_stats": 0, "ce": 0, "colsum_of_logits": 0}
    real_trs, real_ce, real_cs = ops.teacher_row_stats, ops.dino_ce, ops.colsum

    def cs(x, **k):  # (the centre update's own pass over the teacher logits: bf16 [rows, K])
        calls["colsum_of_logits"] += int(x.dtype == torch.bfloat16 and x.shape[-1] == GU.NANO_HEAD["out_dim"])
        return real_cs(x, **k)

    def trs(*a, **k):
        calls["teacher_row_stats"] += 1
        return real_trs(*a, **k)

    def ce(*a, **k):
        calls["ce"] += 1
        calls["ce_with_student_stats"] += int(k.get("s_stats") is not None)
        return real_ce(*a, **k)
    try:
        ops.teacher_row_stats, ops.dino_ce, ops.colsum = trs, ce, cs
        K, B = GU.NANO_HEAD["out_dim"], 64  # rows: student 10 B / 170 B, teacher 2 B / 98 B -- all whole 128-row tiles at B = 64
        crops = _to(GU.make_crops(B, seed=91), dev)

        def fresh():
            torch.manual_seed(5)
            student, teacher = nano_pair()
            loss_fn = L.DDINOLoss(K, 10, 0.04, 0.07, 5, 10).to(dev)
            loss_fn.center.normal_(0, 0.05)
            loss_fn.center_grid.normal_(0, 0.05)
            return student.to(dev), teacher.to(dev), loss_fn
        # (1) the armed step
        student, teacher, loss_fn = fresh()
        tr = engine.EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=0)
        tr.step(crops, 1e-4, 0.04, 0.996, 0)  # (first step: one stream, fills the tables)
        c_armed = (loss_fn.center.clone(), loss_fn.center_grid.clone())
        for k in calls:
            calls[k] = 0
        tr.step(crops, 1e-4, 0.04, 0.996, 0)
        assert L.LOGIT_STATS and calls["teacher_row_stats"] == 0, calls
        assert calls["ce"] >= 2 and calls["ce_with_student_stats"] == calls["ce"], calls
        assert calls["colsum_of_logits"] == 0, calls  # the centre update took the column sums of the teacher heads' GEMMs
        # the first step with the hand-over switched off (same weights, same logits): the centres from the loss's own column sums
        student, teacher, loss_fn = fresh()
        L.LOGIT_STATS = False
        try:
            tr2 = engine.EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=0)
            tr2.step(crops, 1e-4, 0.04, 0.996, 0)
        finally:
            L.LOGIT_STATS = True
        assert calls["colsum_of_logits"] >= 2, calls
        for a, b in zip(c_armed, (loss_fn.center, loss_fn.center_grid)):
            assert (a - b).abs().max().item() < 2e-6 * (1 + b.abs().max().item()), (a - b).abs().max().item()
        # (2) armed forwards, then the centres move before the loss is called: own passes, same value as a loss that was never armed
        student, teacher, loss_fn = fresh()
        with torch.no_grad():
            loss_fn.arm_logit_stats(student, teacher, 0)
            s_out, t_out = student(crops), teacher(crops[:2])
            loss_fn.disarm_logit_stats(student, teacher)
            loss_fn.center.add_(0.01)
            loss_fn.center_grid.sub_(0.02)
            loss_fn._center_version += 1
            for k in calls:
                calls[k] = 0
            armed_then_stale = loss_fn(s_out, t_out, 0).item()
            assert calls["teacher_row_stats"] >= 2, calls  # both teacher levels fell back to their own pass
        student, teacher, loss_fn = fresh()
        with torch.no_grad():
            s_out, t_out = student(crops), teacher(crops[:2])
            loss_fn.center.add_(0.01)
            loss_fn.center_grid.sub_(0.02)
            never_armed = loss_fn(s_out, t_out, 0).item()
        assert abs(armed_then_stale - never_armed) < 1e-6, (armed_then_stale, never_armed)
    finally:
        ops.teacher_row_stats, ops.dino_ce, ops.colsum = real_trs, real_ce, real_cs
        _teardown()


def test_train_one_epoch_drop_in_gpu(lib_built):
    """engine.train_one_epoch (the reference's signature, main_esvit.py:499-501) with the torch.optim.AdamW the unmodified
    train_esvit builds (main_esvit.py:408-411): two batches equal two EsvitTrainer.step calls; the caller's optimizer holds
    the real moments (state_dict() / load_state_dict() round trip = the checkpoint of main_esvit.py:476-488), a resumed run
    continues exactly like an uninterrupted one, and optimizers outside main_esvit.py:408-415 are refused"""
    import argparse
    import esvit_amd.loss as L
    from esvit_amd import engine
    from esvit_amd.update import get_params_groups
    dev = _setup("fp32")
    try:
        K = GU.NANO_HEAD["out_dim"]
        batches = [[c.to(dev) for c in GU.make_crops(2, seed=70 + i)] for i in range(3)]
        # schedules are indexed by the global iteration len(loader) * epoch + it (main_esvit.py:507)
        sched = dict(lr=[3e-4, 2e-4, 1e-4, 9.0], wd=[0.04, 0.05, 0.06, 9.0], mom=[0.99, 0.995, 0.996, 0.0])

        class Loader:
            sampler = None

            def __init__(self, bs):
                self.bs = bs

            def __len__(self):
                return len(self.bs)

            def __iter__(self):
                return iter([(b, None) for b in self.bs])

        def fresh():
            student, teacher = nano_pair()
            student, teacher = student.to(dev), teacher.to(dev)
            loss_fn = L.DDINOLoss(K, 10, 0.04, 0.07, 5, 10).to(dev)
            return student, teacher, loss_fn
        args = argparse.Namespace(clip_grad=3.0, freeze_last_layer=0)
        # (a) the drop-in, three iterations in one epoch, torch AdamW passed by the caller
        student, teacher, loss_fn = fresh()
        opt = torch.optim.AdamW(get_params_groups(student))
        stats = engine.train_one_epoch(student, teacher, teacher, loss_fn, Loader(batches), opt, sched["lr"], sched["wd"], sched["mom"], 0, None, None, args)
        assert set(stats) == {"loss", "lr", "wd"} and stats["loss"] == stats["loss"]
        sd = opt.state_dict()
        n_train = sum(1 for n, p in student.named_parameters() if p.requires_grad and n != "head.last_layer.weight_g")
        assert len(sd["state"]) == n_train and all(float(st["step"]) == 3.0 for st in sd["state"].values())
        assert any(float(st["exp_avg"].abs().max()) > 0 for st in sd["state"].values())
        assert opt.param_groups[0]["lr"] == sched["lr"][2] and opt.param_groups[0]["weight_decay"] == sched["wd"][2]
        # (b) three explicit steps
        s2, t2, l2 = fresh()
        tr = engine.EsvitTrainer(s2, t2, l2, clip_grad=3.0, freeze_last_layer=0)
        losses = [tr.step(b, sched["lr"][i], sched["wd"][i], sched["mom"][i], 0) for i, b in enumerate(batches)]
        assert abs(stats["loss"] - sum(x.item() for x in losses) / 3) < 1e-4  # the epoch mean the reference logs
        # fp32 atomics in the bias-table gradient scatter make two runs differ in the last bits of a few gradients, and an Adam
        # step moves an entry whose gradient is ~0 by up to +-lr whatever its magnitude: compare the three-step UPDATE as a
        # vector (relative L2 distance) instead of entry by entry
        init_s, init_t = fresh()[:2]
        init_s, init_t = dict(init_s.named_parameters()), dict(init_t.named_parameters())

        def same_update(tag, pa, pb, init, tol):
            for (n, a), (_, b) in zip(pa, pb):
                ua, ub = (a - init[n]).detach(), (b - init[n]).detach()
                assert (ua - ub).norm().item() <= tol * ub.norm().item() + 1e-9, (tag, n, (ua - ub).norm().item(), ub.norm().item())
        same_update("student", student.named_parameters(), s2.named_parameters(), init_s, 2e-2)
        same_update("teacher", teacher.named_parameters(), t2.named_parameters(), init_t, 2e-3)
        # (c) resume: two iterations, checkpoint (the dict of main_esvit.py:476-488 through torch.save), fresh objects,
        # load, third iteration == the uninterrupted run
        import io
        s3, t3, l3 = fresh()
        o3 = torch.optim.AdamW(get_params_groups(s3))
        two = Loader(batches[:2])
        engine.train_one_epoch(s3, t3, t3, l3, two, o3, sched["lr"], sched["wd"], sched["mom"], 0, None, None, args)
        buf = io.BytesIO()
        torch.save({"student": s3.state_dict(), "teacher": t3.state_dict(), "optimizer": o3.state_dict(), "dino_loss": l3.state_dict()}, buf)
        buf.seek(0)
        ck = torch.load(buf, map_location="cpu")
        s4, t4, l4 = fresh()
        o4 = torch.optim.AdamW(get_params_groups(s4))
        s4.load_state_dict(ck["student"]), t4.load_state_dict(ck["teacher"]), o4.load_state_dict(ck["optimizer"]), l4.load_state_dict(ck["dino_loss"])
        one = Loader(batches[2:])
        # the global iteration of the resumed epoch: len(loader) * epoch + it with len 1 -> shift the schedules accordingly
        engine.train_one_epoch(s4, t4, t4, l4, one, o4, sched["lr"][2:], sched["wd"][2:], sched["mom"][2:], 0, None, None, args)
        same_update("resume", student.named_parameters(), s4.named_parameters(), init_s, 2e-2)
        assert all(float(st["step"]) == 3.0 for st in o4.state_dict()["state"].values())
        # (d) anything train_esvit cannot build (AdamW / SGD / LARS) is refused instead of silently ignored
        with pytest.raises(TypeError):
            engine.train_one_epoch(s4, t4, t4, l4, one, torch.optim.Adam(s4.parameters(), lr=0.1), sched["lr"][2:], sched["wd"][2:], sched["mom"][2:], 0, None, None, args)
        # (e) the --use_fp16 protocol (main_esvit.py:417-419, 576-584): GradScaler.scale / unscale_ / step / update around the
        # fused update.  Power-of-two scales are exact, so the scaled run equals the plain one; the scale grows on schedule.
        s5, t5, l5 = fresh()
        o5 = torch.optim.AdamW(get_params_groups(s5))
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=2)
        st5 = engine.train_one_epoch(s5, t5, t5, l5, Loader(batches), o5, sched["lr"], sched["wd"], sched["mom"], 0, None, scaler, args)
        assert abs(st5["loss"] - stats["loss"]) < 1e-4
        same_update("scaler student", student.named_parameters(), s5.named_parameters(), init_s, 2e-2)
        same_update("scaler teacher", teacher.named_parameters(), t5.named_parameters(), init_t, 2e-3)
        assert scaler.get_scale() == 2.0 ** 11  # three finite steps, growth interval 2
        assert all(float(st["step"]) == 3.0 for st in o5.state_dict()["state"].values())
        # a non-finite gradient: the optimizer step is skipped (student and moments untouched, scale halved), the EMA still runs
        before_s = {n: p.detach().clone() for n, p in s5.named_parameters()}
        before_t = {n: p.detach().clone() for n, p in t5.named_parameters()}
        victim = dict(s5.named_parameters())["layers.0.blocks.0.mlp.fc1.bias"]
        h = victim.register_hook(lambda g: g + float("inf"))
        engine.train_one_epoch(s5, t5, t5, l5, Loader(batches[:1]), o5, sched["lr"], sched["wd"], sched["mom"], 0, None, scaler, args)
        h.remove()
        assert scaler.get_scale() == 2.0 ** 10
        m = sched["mom"][0]
        for n, p in s5.named_parameters():
            assert torch.equal(p, before_s[n]), n
        for (n, p), (_, q) in zip(t5.named_parameters(), s5.named_parameters()):
            assert torch.allclose(p, before_t[n] * m + q.detach() * (1 - m), rtol=1e-5, atol=1e-7), n
        assert all(float(st["step"]) == 3.0 for st in o5.state_dict()["state"].values())
    finally:
        _teardown()


def test_trainer_step_with_logit_statistics_from_the_gemm(lib_built, monkeypatch):
    """engine.EsvitTrainer.step with the heads' last-layer GEMMs emitting the loss's softmax statistics (the default) vs the same
    steps with the loss computing them in its own passes (ESVIT_LOGIT_STATS=0): B = 128 so that every logit tensor comes in whole
    128-row tiles; the statistics path must actually be taken (no esvit_teacher_row_stats call), the first loss agrees to 1e-6 relative, the
    next two (after updates) to 1e-3, parameters after three steps to the AdamW step bound"""
    import esvit_amd
    import esvit_amd.loss as L
    from esvit_amd import ops
    from esvit_amd import params as P
    from esvit_amd.engine import EsvitTrainer
    dev = _setup("bf16")
    calls = {"t": 0}
    f0 = ops.teacher_row_stats
    monkeypatch.setattr(ops, "teacher_row_stats", lambda *a, **k: (calls.__setitem__("t", calls["t"] + 1), f0(*a, **k))[1])

    def run(on):
        monkeypatch.setattr(L, "LOGIT_STATS", on)
        P.clear()
        student, teacher = nano_pair()
        student, teacher = student.to(dev), teacher.to(dev)
        loss_fn = L.DDINOLoss(GU.NANO_HEAD["out_dim"], 10, 0.04, 0.07, 5, 10).to(dev)
        tr = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=0)
        calls["t"] = 0
        losses = [tr.step(_to(GU.make_crops(128, seed=40 + i), dev), 5e-4, 0.04, 0.996, epoch=i).item() for i in range(3)]
        torch.cuda.synchronize()
        tr.reducer.close()
        return losses, {k: v.detach().float().clone() for k, v in student.state_dict().items()}, calls["t"]

    try:
        l_on, p_on, n_on = run(True)
        l_off, p_off, n_off = run(False)
        assert n_on == 0 and n_off == 6, (n_on, n_off)
        # same parameters in step 1: the two losses differ by fp32 summation order only; afterwards the updates have diverged by
        # the sign flips of near-zero gradients under AdamW
        assert abs(l_on[0] - l_off[0]) / abs(l_off[0]) < 1e-6, (l_on, l_off)
        assert max(abs(a - b) / abs(b) for a, b in zip(l_on, l_off)) < 1e-3, (l_on, l_off)
        # AdamW's normalised step is bounded by lr per element and step (a near-zero gradient may flip sign: 2 lr per step)
        assert max((p_on[k] - p_off[k]).abs().max().item() for k in p_on if p_on[k].numel()) < 6 * 5e-4
    finally:
        _teardown()


@pytest.mark.parametrize("arch,B", [("swin_tiny_w7", 32), ("swin_tiny_w14", 16), ("deit_small", 32), ("cvt_s1", 32), ("vil_tiny", 32)])
def test_full_width_bf16_tracks_fp32_mode(arch, B):
    """The bench configurations at FULL width and a batch that fills every CU (>= 1024 window-heads in the attention kernels), three
    steps in bf16 against the fp32 mode of the same library -- mostly disjoint kernels, the same math.  The fixtures of the reference
    stop at batch 2-4 per crop; this is the check that runs at the occupancy of the bench lines (the head_dim-64 attention store of
    round 4 passed every small-geometry test and poisoned every step of the ViT / CvT / ViL benches).  Observed on MI355X
    (tools/probe/diag_prec.py): loss differences 4e-5 .. 1.2e-4.  (The comparison with the CPU oracle at this occupancy is
    test_bench_occupancy_step_matches_oracle below.)"""
    import bench
    import esvit_amd
    from esvit_amd.engine import EsvitTrainer
    dev = torch.device("cuda:0")
    res = {}
    try:
        for prec in ("fp32", "bf16"):
            esvit_amd.set_precision(prec)
            torch.manual_seed(0)
            student, teacher, loss_fn = bench.build(dev, 0.0, arch)
            trainer = EsvitTrainer(student, teacher, loss_fn, clip_grad=3.0, freeze_last_layer=1, teacher_stream=False)
            crops = [c.to(dev) for c in GU.make_crops(B, seed=1234)]
            losses = [trainer.step(crops, 5e-4 * B / 256.0, 0.04, 0.996, 1).item() for _ in range(3)]
            norm = torch.sqrt(sum((p.detach().float() ** 2).sum() for p in student.parameters())).item()
            assert trainer.updater.take_skipped() == 0
            res[prec] = (losses, norm)
            del student, teacher, loss_fn, trainer, crops
            torch.cuda.empty_cache()
    finally:
        esvit_amd.set_precision("bf16")
    for a, b in zip(res["fp32"][0], res["bf16"][0]):
        assert a == a and b == b and abs(a - b) < 4e-4, (arch, res)
    # three AdamW steps move every parameter by <= 3 lr whatever the precision: the parameter norms of the two modes stay together
    # (the bound is 20x the largest difference observed on MI355X, profiles/r06_parity_observed.jsonl)
    d_norm = abs(res["fp32"][1] - res["bf16"][1]) / res["fp32"][1]
    GU.record_parity(test="full_width_bf16_vs_fp32_mode", arch=arch, B=B, d_loss=max(abs(a - b) for a, b in zip(res["fp32"][0], res["bf16"][0])),
                     d_param_norm_rel=d_norm)
    assert d_norm < 1e-4, (arch, d_norm)



@pytest.mark.parametrize("arch,B,ragged", [
    pytest.param("swin_tiny_w7", 32, None, id="swin_tiny_w7-32"), pytest.param("swin_base_w14", 8, None, id="swin_base_w14-8"),
    pytest.param("deit_small", 16, None, id="deit_small-16"), pytest.param("cvt_s1", 16, None, id="cvt_s1-16"), pytest.param("vil_tiny", 16, None, id="vil_tiny-16"),
    # one backbone pass per resolution group (SwinBlockFn, vit_block) instead of the model's default route
    pytest.param("swin_tiny_w7", 32, False, id="swin_tiny_w7-32-per_group"), pytest.param("deit_small", 16, False, id="deit_small-16-per_group")])
def test_weight_gradient_stream_is_bit_identical_to_inline(arch, B, ragged, lib_built):
    """functional._side_run launches the weight-gradient GEMMs of a backward node on a side stream and joins before the node returns.  The
    same kernels on the same operands in a different launch order: every gradient of one backward must equal, bit for bit, the gradient
    with the GEMMs in line (ESVIT_WGRAD_STREAM=0) -- at a batch that fills every CU, and repeated, so that a missing dependency (an operand
    read before its producer finished, a buffer re-used while the side stream still reads it) shows up as a difference"""
    import bench
    import esvit_amd
    import esvit_amd.functional as F
    dev = torch.device("cuda:0")
    esvit_amd.set_precision("bf16")
    was = F.WGRAD_STREAM
    try:
        torch.manual_seed(0)
        student, teacher, loss_fn = bench.build(dev, 0.0, arch)
        if ragged is not None:
            assert hasattr(student, "ragged_multi_crop")
            student.ragged_multi_crop = ragged
        crops = [c.to(dev) for c in GU.make_crops(B, seed=77)]
        with torch.no_grad():
            t_out = teacher(crops[:2])

        state = {k: v.clone() for k, v in loss_fn.state_dict().items()}  # (the loss moves its centres in every forward)

        def grads(on):
            F.WGRAD_STREAM = on
            loss_fn.load_state_dict(state)
            torch.cuda.synchronize()
            for p in student.parameters():
                p.grad = None
            loss = loss_fn(student(crops), t_out, 1, None)
            loss.backward()
            torch.cuda.synchronize()
            return loss.item(), {n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}

        l_ref, g_ref = grads(False)
        l_ref2, g_ref2 = grads(False)
        assert l_ref == l_ref and len(g_ref) > 50
        # (tensors whose gradient is summed with float atomics are not bit-reproducible even in line: those are compared to 1e-5 of their range)
        exact = [n for n in g_ref if torch.equal(g_ref[n], g_ref2[n])]
        assert len(exact) >= 0.9 * len(g_ref), (arch, len(exact), len(g_ref))
        for rep in range(4):
            l_on, g_on = grads(True)
            assert abs(l_on - l_ref) <= abs(l_ref2 - l_ref) + 1e-6
            assert g_on.keys() == g_ref.keys()
            bad = [n for n in exact if not torch.equal(g_on[n], g_ref[n])]
            assert not bad, (arch, rep, bad[:5])
            for n in g_ref:
                if n not in exact:
                    scale = g_ref[n].abs().max().item() + 1e-30
                    assert (g_on[n] - g_ref[n]).abs().max().item() <= 1e-5 * scale, (arch, rep, n)
        assert any(st["stream"] is not None for st in F._wg_state.values())  # (the side stream was really in use)
    finally:
        F.WGRAD_STREAM = was
        _teardown()


ORACLE_SWIN = {"swin_tiny_w7": GU.SWIN_T,
               "swin_tiny_w14": dict(embed_dim=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), window=14, img=224),
               "swin_base_w14": dict(embed_dim=128, depths=(2, 2, 18, 2), heads=(4, 8, 16, 32), window=14, img=224)}


def _oracle_forward(arch):
    if arch in ORACLE_SWIN:
        return lambda w, c: O.swin_multicrop(w, c, ORACLE_SWIN[arch])
    if arch == "deit_small":
        return lambda w, c: O.vit_multicrop(w, c, dict(depth=12, heads=6, patch=16))
    return lambda w, c: O.cvt_multicrop(w, c, dict(dims=(64, 192, 384, 768), heads=(1, 3, 6, 12), depths=(2, 2, 6, 2)))  # (s1.yaml)


def _oracle_step(arch, student, teacher, crops, K):
    """one forward / loss / backward of the CPU oracle (oracle/esvit_oracle.py, fp32, host threads) on the given modules' weights
    -> (student outputs, loss, {parameter name: gradient})"""
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in student.state_dict().items()}
    td = {k: v.detach().cpu().clone() for k, v in teacher.state_dict().items()}
    fwd = _oracle_forward(arch)
    s_ref = fwd(sd, crops)
    with torch.no_grad():
        t_ref = fwd(td, crops[:2])
    c0 = torch.zeros(1, K)
    l_ref, _, _ = O.ddino_loss(s_ref, t_ref, c0, c0, O.teacher_temp(0, 0.04, 0.04, 0, 1), 10)
    l_ref.backward()
    return s_ref, l_ref.item(), {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}


# parameters whose gradients are compared ELEMENT by element with the oracle's (a strided sample of each tensor): the first parameter
# whose name contains the key.  Norms alone (the round-5 form of this test) would pass a permutation or a sign error inside a tensor.
GRAD_PROBE_KEYS = ("patch_embed", "relative_position_bias_table", "qkv.bias", "layers.2.blocks.1.attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight",
                   "layers.2.blocks.4.mlp.fc2.weight", "downsample.reduction.weight", "norm1.weight", "head.mlp.0.weight", "head_dense.last_layer.weight_v",
                   "blocks.3.attn.qkv.weight", "pos_embed", "cls_token", "conv_proj_q")
GRAD_PROBE_N = 8192


def _grad_probes(named_grads, g_ref):
    """-> [(name, max |g - g_ref| / max |g_ref| over the sample, cosine of the two samples)]"""
    names = list(named_grads)
    picked = []
    for key in GRAD_PROBE_KEYS:
        for n in names:
            if key in n and n not in picked and n in g_ref:
                picked.append(n)
                break
    # a backbone whose parameter names match few of the keys (CvT: stageN.M.layers...): fill up to ten tensors at regular strides of the name list
    rest = [n for n in sorted(names) if n not in picked and n in g_ref and g_ref[n].numel() >= 64]
    while len(picked) < 10 and rest:
        picked.append(rest.pop((len(rest) * 5) // 11))
    out = []
    for n in picked:
        a = named_grads[n].detach().float().cpu().reshape(-1)
        b = g_ref[n].detach().float().reshape(-1)
        st = max(1, a.numel() // GRAD_PROBE_N)
        a, b = a[::st].double(), b[::st].double()
        scale = b.abs().max().item() + 1e-30
        cos = (a @ b / (a.norm() * b.norm() + 1e-30)).item()
        out.append((n, ((a - b).abs().max().item() / scale), cos))
    return out


@pytest.mark.parametrize("arch,B,K", [("swin_tiny_w7", 32, 65536), ("swin_tiny_w14", 16, 8192), ("swin_base_w14", 8, 8192), ("deit_small", 16, 8192),
                                      ("cvt_s1", 16, 8192)])
def test_bench_occupancy_step_matches_oracle(arch, B, K, lib_built):
    """One forward / loss / backward at FULL width and a batch that fills every CU (B = 32: 1024-4096 window-heads per attention launch,
    the fused attention branch with 16 window groups per workgroup; W14: 14x14 windows with dead query tiles on the 96^2 crops' 6x6 / 12x12
    maps) on the HIP path, fp32 mode and bf16 mode, against the CPU oracle on the same weights and crops -- not against another mode of
    this library.  drop_path 0.  Bounds: |loss delta| <= 1e-4 (fp32) / 1e-3 (bf16); gradient norms of every parameter within 5e-3 (fp32) /
    4 % (bf16) of the oracle's; ELEMENT-wise, a strided sample of >= 6 gradient tensors (GRAD_PROBE_KEYS: patch embedding, relative-position
    table, qkv bias, qkv / proj / fc1 / fc2 / merge weights, a LayerNorm weight, both heads) within 5e-3 (fp32) / 0.2 (bf16) of the tensor's
    largest entry and at cosine >= 0.99999 / 0.99 with the oracle's sample (observed: 6e-6 and 1 - 2e-11 in fp32 mode on the Swin configurations -- the index
    check --, 1.2e-3 / 1 - 3.5e-7 on a CvT LayerNorm weight whose gradient is a long cancelling sum; 0.05-0.13 and
    0.996-0.9985 in bf16 mode, the rounding noise of a gradient that crossed twelve blocks); the first student logits within 1e-3 / 8e-2 of their range.
    (Observed values: profiles/r06_parity_observed.jsonl.)"""
    import esvit_amd
    if arch == "deit_small":
        from esvit_amd.models import vision_transformer as V
    torch.manual_seed(0)
    cpu_threads = torch.get_num_threads()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    try:
        def make(seed, is_teacher):
            if arch != "deit_small":
                from esvit_amd import config as CFG
                m = esvit_amd.build_model(CFG.model_config(arch, DROP_PATH_RATE=0.0), is_teacher=is_teacher, use_dense_prediction=True)
                width = m.num_features
            else:
                m = V.deit_small(patch_size=16, drop_path_rate=0.0, use_dense_prediction=True)
                width = m.embed_dim
            m.head, m.head_dense = esvit_amd.DINOHead(width, K, norm_last_layer=True), esvit_amd.DINOHead(width, K, norm_last_layer=False)
            GU.fill_state_dict(m.state_dict(), seed)
            return m
        student, teacher = make(61, False), make(62, True)
        student.head.last_layer.weight_g.data.fill_(1)
        for p in teacher.parameters():
            p.requires_grad = False
        crops = GU.make_crops(B, seed=93)
        s_ref, l_ref, g_ref = _oracle_step(arch, student, teacher, crops, K)
        for prec in ("fp32", "bf16"):
            dev = _setup(prec)
            try:
                st, te = student.to(dev), teacher.to(dev)
                for p in st.parameters():
                    p.grad = None
                loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.04, 0, 1).to(dev)
                dcrops = [c.to(dev) for c in crops]
                with torch.no_grad():
                    t_out = te(dcrops[:2])
                s_out = st(dcrops)
                loss = loss_fn(s_out, t_out, 0, None)
                loss.backward()
                loss_fn.synchronize()
                fp = prec == "fp32"
                d_loss = abs(loss.item() - l_ref)
                d_out = ((s_out[0].float().cpu() - s_ref[0].detach()).abs().max() / (s_ref[0].detach().abs().max() + 1e-12)).item()
                floor = 1e-5 * max(g.norm().item() for g in g_ref.values())
                worst, wname = 0.0, None
                for n, p in st.named_parameters():
                    if not p.requires_grad:
                        continue
                    r = g_ref[n].norm().item()
                    rel = abs(p.grad.float().norm().item() - r) / max(r, floor)
                    if rel > worst:
                        worst, wname = rel, n
                probes = _grad_probes({n: p.grad for n, p in st.named_parameters() if p.requires_grad and p.grad is not None}, g_ref)
                if fp:
                    # a gradient that is a long CANCELLING sum (CvT: the LayerNorm weight in front of the BatchNorm'd conv projections) shows up in fp32
                    # mode as an error ~200x the others (1.2e-3 vs 6e-6: summation order); bf16 rounding of its terms then leaves no signal at all
                    # (cosine 0.66).  Such tensors are checked in fp32 mode only.
                    ill_conditioned = {n for n, e, _ in probes if e > 1e-4}
                else:
                    probes = [t for t in probes if t[0] not in ill_conditioned]
                w_el = max(probes, key=lambda t: t[1])
                w_cos = min(probes, key=lambda t: t[2])
                GU.record_parity(test="bench_occupancy_vs_oracle", arch=arch, B=B, K=K, prec=prec, loss=loss.item(), loss_ref=l_ref, d_loss=d_loss, d_logits=d_out,
                                 worst_grad_norm_rel=worst, worst_grad=wname, n_grad_probes=len(probes), worst_grad_elem_rel=w_el[1], worst_grad_elem=w_el[0],
                                 worst_grad_cos=w_cos[2], worst_grad_cos_name=w_cos[0])
                assert math.isfinite(loss.item()) and d_loss <= (1e-4 if fp else 1e-3), (arch, prec, loss.item(), l_ref)
                assert d_out <= (1e-3 if fp else 8e-2), (arch, prec, d_out)
                assert worst <= (5e-3 if fp else 4e-2), (arch, prec, wname, worst)
                assert len(probes) >= 6, probes
                assert w_el[1] <= (5e-3 if fp else 0.2), (arch, prec, probes)
                assert w_cos[2] >= (0.99999 if fp else 0.99), (arch, prec, probes)
                del loss_fn, dcrops, t_out, s_out, loss
            finally:
                _teardown()
            student, teacher = st.cpu(), te.cpu()
    finally:
        torch.set_num_threads(cpu_threads)


def test_bench_batch_forward_loss_matches_oracle(lib_built):
    """The bench line's own occupancy: B = 128, Swin-T W7, 2 x 224^2 + 8 x 96^2 crops, out_dim 65536 (87040 stage-2 token rows, 21760 x 65536
    dense-head logits), teacher forward + student forward + DDINOLoss in bf16 mode against the CPU oracle's forward on the same weights and
    crops (no backward: the oracle's B = 128 backward does not fit the few-minutes budget; gradients at full width are compared at B = 32
    above).  |loss delta| <= 1e-3 (north_star's tolerance).  On a host with less than 40 GiB of free memory the oracle leg runs at
    out_dim 8192 instead (its fp32 logits at 65536 need ~20 GiB)."""
    import esvit_amd
    from esvit_amd import config as CFG
    free = 0
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable"):
                    free = int(line.split()[1]) // (1 << 20)
    except OSError:
        pass
    K, B = (65536 if free >= 40 else 8192), 128
    cpu_threads = torch.get_num_threads()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    try:
        def make(seed, is_teacher):
            m = esvit_amd.build_model(CFG.model_config("swin_tiny_w7", DROP_PATH_RATE=0.0), is_teacher=is_teacher, use_dense_prediction=True)
            m.head, m.head_dense = esvit_amd.DINOHead(m.num_features, K, norm_last_layer=True), esvit_amd.DINOHead(m.num_features, K, norm_last_layer=False)
            GU.fill_state_dict(m.state_dict(), seed)
            return m
        student, teacher = make(71, False), make(72, True)
        crops = GU.make_crops(B, seed=97)
        with torch.no_grad():
            fwd = _oracle_forward("swin_tiny_w7")
            sd = {k: v.detach().clone() for k, v in student.state_dict().items()}
            td = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
            t_ref = fwd(td, crops[:2])
            s_ref = fwd(sd, crops)
            c0 = torch.zeros(1, K)
            l_ref = O.ddino_loss(s_ref, t_ref, c0, c0, O.teacher_temp(0, 0.04, 0.04, 0, 1), 10)[0].item()
            cls_ref = s_ref[0][:8].clone()
            del t_ref, s_ref, sd, td
        dev = _setup("bf16")
        try:
            st, te = student.to(dev), teacher.to(dev)
            loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.04, 0, 1).to(dev)
            dcrops = [c.to(dev) for c in crops]
            with torch.no_grad():
                t_out = te(dcrops[:2])
                s_out = st(dcrops)
                loss = loss_fn(s_out, t_out, 0, None)
            loss_fn.synchronize()
            d_loss = abs(loss.item() - l_ref)
            d_out = ((s_out[0][:8].float().cpu() - cls_ref).abs().max() / (cls_ref.abs().max() + 1e-12)).item()
            GU.record_parity(test="bench_batch_forward_vs_oracle", arch="swin_tiny_w7", B=B, K=K, prec="bf16", loss=loss.item(), loss_ref=l_ref, d_loss=d_loss,
                             d_logits=d_out)
            assert math.isfinite(loss.item()) and d_loss <= 1e-3, (loss.item(), l_ref)
            assert d_out <= 8e-2, d_out
        finally:
            _teardown()
    finally:
        torch.set_num_threads(cpu_threads)
