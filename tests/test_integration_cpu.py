"""Integration level 1: OUR build_model / DINOHead / DDINOLoss objects behind the training loop of
main_esvit.py:499-600 -- torch.optim.AdamW over utils.get_params_groups, utils.clip_gradients, utils.cancel_gradients_last_layer, the
positional EMA zip and a DistributedDataParallel wrap -- end with the same loss, parameters, teacher and centres as the reference's own
modules behind its own UNMODIFIED loop.  Then the checkpoint dict of main_esvit.py:476-488 is exchanged in both directions.

The reference side is recorded in tests/golden/level1.pt (oracle/gen_golden.py `level1`: the reference's train_one_epoch compiled from
its source, its utils, its modules): the epoch's stats, every parameter update of student and teacher (a seeded, name-keyed sample of
1024 entries of the larger tensors, GU.level1_index), the centres, the optimizer's groups and state, and the structure of the checkpoint
its utils.save_on_master wrote.  Here the loop is the restatement below, run on our objects; its agreement with the recorded reference
run is part of what is checked.

CPU only: the kernels are replaced by their torch restatement (oracle/ops_ref.py), the host code under test is the product's.  The
caller's fp32 branch references an undefined name (`model`, main_esvit.py:571) whenever --clip_grad > 0, so the reference ran its
scaler branch with the duck-typed no-op scaler documented in SURVEY.md 8b hazard (i); the restatement follows that branch."""
import os

import pytest
import torch

from oracle import ref_loader as RL
from tests import golden_utils as GU
from tests.test_composition_cpu import cpu_ops, nano_pair  # noqa: F401  (fixture)
from tests.test_oracle_cpu import GOLD


class NoOpScaler:
    """what a caller passes as fp16_scaler to take the (bug-free) scaler branch of main_esvit.py:576-584 without fp16"""

    def scale(self, loss):
        return loss

    def unscale_(self, optimizer):
        pass

    def step(self, optimizer):
        optimizer.step()

    def update(self):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


class Loader:
    sampler = None

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter([(b, None) for b in self.batches])


@pytest.fixture(scope="module")
def level1():
    return torch.load(os.path.join(GOLD, "level1.pt"), weights_only=False)


@pytest.fixture()
def process_group():
    """the single-process gloo group DDP needs (world 1), taken down again if this test made it: later tests see no group"""
    import torch.distributed as dist
    made = not dist.is_initialized()
    RL.ensure_single_process_group()
    yield
    if made:
        dist.destroy_process_group()


def get_params_groups(model):
    """utils.get_params_groups (utils.py:672-683): biases and 1-d tensors form the second group, without weight decay"""
    regularized, not_regularized = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (not_regularized if n.endswith(".bias") or p.ndim == 1 else regularized).append(p)
    return [{"params": regularized}, {"params": not_regularized, "weight_decay": 0.0}]


def train_one_epoch(student, teacher, loss_fn, batches, optimizer, epoch, clip_grad, freeze_last_layer, scaler):
    """main_esvit.py:499-600, scaler branch: per iteration the schedule values into the param groups (weight decay into the first one
    only), teacher forward on the two global crops, student forward on all, loss, scaled backward, unscale, per-parameter gradient clip
    (utils.clip_gradients), last-layer gradients dropped before epoch freeze_last_layer (utils.cancel_gradients_last_layer), optimizer
    step through the scaler, EMA of the teacher over zip(student.module.parameters(), teacher.parameters()); returns the epoch means of
    loss, lr and wd (the metric logger's global_avg).  The iterations are those of GU.LEVEL1_SCHED."""
    sch = GU.LEVEL1_SCHED
    seen = {"loss": [], "lr": [], "wd": []}
    for it, images in enumerate(batches):
        for i, group in enumerate(optimizer.param_groups):
            group["lr"] = sch["lr"][it]
            if i == 0:
                group["weight_decay"] = sch["wd"][it]
        teacher_output = teacher(images[:2])
        student_output = student(images)
        loss = loss_fn(student_output, teacher_output, epoch, None)
        assert torch.isfinite(loss)
        optimizer.zero_grad()
        scaler.scale(loss).backward()
        scaler.unscale_(optimizer)
        for _, p in student.named_parameters():
            if p.grad is not None:
                coef = clip_grad / (p.grad.data.norm(2) + 1e-6)
                if coef < 1:
                    p.grad.data.mul_(coef)
        if epoch < freeze_last_layer:
            for n, p in student.named_parameters():
                if "last_layer" in n:
                    p.grad = None
        scaler.step(optimizer)
        scaler.update()
        with torch.no_grad():
            m = sch["mom"][it]
            for q, k in zip(student.module.parameters(), teacher.parameters()):
                k.data.mul_(m).add_((1 - m) * q.detach().data)
        seen["loss"].append(loss.item())
        seen["lr"].append(optimizer.param_groups[0]["lr"])
        seen["wd"].append(optimizer.param_groups[0]["weight_decay"])
    return {k: sum(v) / len(v) for k, v in seen.items()}


def restart_from_checkpoint(path, run_variables=None, **kwargs):
    """utils.restart_from_checkpoint (utils.py:126-163): every named object loads its entry (strict=False where the method takes it),
    run_variables are filled from the checkpoint"""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    for key, value in kwargs.items():
        if key in ckpt and value is not None:
            try:
                value.load_state_dict(ckpt[key], strict=False)
            except TypeError:
                value.load_state_dict(ckpt[key])
    for key in run_variables or {}:
        if key in ckpt:
            run_variables[key] = ckpt[key]


def _run(student, teacher, loss_fn, batches):
    from torch.nn.parallel import DistributedDataParallel as DDP
    ddp = DDP(student)  # main_esvit.py:377 (gloo, world 1 here)
    opt = torch.optim.AdamW(get_params_groups(ddp))  # main_esvit.py:408-411
    stats = train_one_epoch(ddp, teacher, loss_fn, batches, opt, 1, 3.0, 1, NoOpScaler())
    return ddp, opt, stats


def _check_against_reference(gold, ddp, teacher, loss_fn, opt, stats, init_s, init_t):
    """(a) ours behind the loop against (b) the reference's modules behind its own loop, same weights and crops"""
    assert set(stats) == set(gold["stats"]) == {"loss", "lr", "wd"}
    assert abs(stats["loss"] - gold["stats"]["loss"]) < 1e-4, (stats, gold["stats"])
    assert stats["lr"] == pytest.approx(gold["stats"]["lr"]) and stats["wd"] == pytest.approx(gold["stats"]["wd"])
    assert [n for n, _ in ddp.module.named_parameters()] == gold["names"]
    # two AdamW steps: the first one moves every entry by ~lr * sign(g), so an entry whose gradient is ~0 can land a whole step
    # apart under fp32 round-off; what must agree is the update as a vector (relative L2 distance of the parameter deltas)
    ua_s = GU.level1_updates(ddp.module, init_s)
    for n, ub in gold["student"].items():
        ua = ua_s[n]
        if ub.norm() > 0:
            assert (ua - ub).norm() <= 2e-2 * ub.norm(), (n, (ua - ub).norm().item(), ub.norm().item())
        else:
            assert torch.equal(ua, ub), n  # untouched on both sides (last layer during the freeze epoch would be; frozen weight_g)
    ua_t = GU.level1_updates(teacher, init_t)
    for n, ub in gold["teacher"].items():
        ua = ua_t[n]
        assert (ua - ub).norm() <= 1e-3 * ub.norm() + 1e-9, (n, (ua - ub).norm().item(), ub.norm().item())
    assert torch.allclose(loss_fn.center, gold["center"], atol=1e-6) and torch.allclose(loss_fn.center_grid, gold["center_grid"], atol=1e-6)
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == gold["opt_groups"] and sorted(sd["state"]) == gold["opt_state_keys"]


def test_level1_unmodified_train_one_epoch_and_checkpoints(cpu_ops, tmp_path, level1, process_group):  # noqa: F811
    import esvit_amd
    gold = level1["swin"]
    K = GU.NANO_HEAD["out_dim"]
    batches = [GU.make_crops(2, seed=70 + i) for i in range(2)]
    student, teacher = nano_pair()
    loss_fn = esvit_amd.DDINOLoss(K, 10, 0.04, 0.07, 5, 10)
    ddp, opt, stats = _run(student, teacher, loss_fn, batches)
    init_s, init_t = nano_pair()
    _check_against_reference(gold, ddp, teacher, loss_fn, opt, stats, dict(init_s.named_parameters()), dict(init_t.named_parameters()))

    # (c) the checkpoint dict of main_esvit.py:476-488, both directions
    ckpt = {"student": ddp.state_dict(), "teacher": teacher.state_dict(), "optimizer": opt.state_dict(), "epoch": 2,
            "dino_loss": loss_fn.state_dict(), "fp16_scaler": {}}
    ours_ckpt, ref_ckpt = os.path.join(tmp_path, "ours.pth"), os.path.join(tmp_path, "ref.pth")
    torch.save(ckpt, ours_ckpt)
    # ours -> the reference's modules: what we write has the structure of what the reference wrote -- every key, shape and dtype of
    # student, teacher, optimizer (groups with their hyper-parameters, state) and loss -- so its strict loads take it as its own
    assert GU.layout(torch.load(ours_ckpt, weights_only=False)) == gold["ckpt_layout"]
    # reference -> our modules: a checkpoint of exactly the reference's structure restores into fresh objects of ours
    ref = GU.materialize(gold["ckpt_layout"], seed=3)
    torch.save(ref, ref_ckpt)

    def fresh_ours():
        from torch.nn.parallel import DistributedDataParallel as DDP
        s, t = nano_pair()
        for p in s.parameters():
            p.data.zero_()
        d = DDP(s)
        return d, t, torch.optim.AdamW(get_params_groups(d)), esvit_amd.DDINOLoss(K, 10, 0.04, 0.07, 5, 10)

    def same(sa, sb):
        assert list(sa.keys()) == list(sb.keys())
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k

    d, t, o, lf = fresh_ours()
    to_restore = {"epoch": 0}
    restart_from_checkpoint(ref_ckpt, run_variables=to_restore, student=d, teacher=t, optimizer=o, fp16_scaler=NoOpScaler(), dino_loss=lf)
    assert to_restore["epoch"] == 2
    same(d.state_dict(), ref["student"])
    same(t.state_dict(), ref["teacher"])
    same(lf.state_dict(), ref["dino_loss"])
    assert sorted(o.state_dict()["state"]) == sorted(ref["optimizer"]["state"])
    k0 = gold["exp_avg0"][0]
    assert torch.equal(o.state_dict()["state"][k0]["exp_avg"], ref["optimizer"]["state"][k0]["exp_avg"])


def test_level1_vit_behind_unmodified_train_one_epoch(cpu_ops, tmp_path, level1, process_group):  # noqa: F811
    """the same for the monolithic ViT (the reference's default --arch, main_esvit.py:305-327): our VisionTransformer + DINOHeads +
    DDINOLoss behind the loop end with the loss and the parameter updates of the reference's own ViT behind its own"""
    import esvit_amd
    from tests.test_vit_cpu import nano_vit_pair
    gold = level1["vit"]
    K = GU.NANO_HEAD["out_dim"]
    batches = [GU.make_crops(2, n_local=3, sizes=GU.NANO_VIT["sizes"], seed=80 + i) for i in range(2)]
    student, teacher = nano_vit_pair()
    loss_fn = esvit_amd.DDINOLoss(K, 5, 0.04, 0.07, 5, 10)
    ddp, opt, stats = _run(student, teacher, loss_fn, batches)
    init_s, init_t = nano_vit_pair()
    _check_against_reference(gold, ddp, teacher, loss_fn, opt, stats, dict(init_s.named_parameters()), dict(init_t.named_parameters()))
    # checkpoints are interchangeable: the reference's ViT (its state dict as its checkpoint holds it) loads ours
    want = {k[len("module."):]: v for k, v in gold["ckpt_layout"]["student"].items()}
    assert GU.layout(ddp.module.state_dict()) == want
