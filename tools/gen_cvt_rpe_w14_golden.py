"""Generate tests/golden/nano_cvt_rpe_w14.pt from the REFERENCE's own modules (needs the reference tree, oracle/ref_loader.py):

    python tools/gen_cvt_rpe_w14_golden.py

experiments/imagenet/cvt_v4/res_stem/s1_rpe_w14.yaml in miniature: residual stem, 14x14 windows at head_dim 64 WITH relative-position
tables on the first stage, 7x7 on the second.  Crops 112 / 64 -> maps 28, 14 / 16 (padded to 28), 8 (padded to 14).  One training step
through the reference, by the recipe of oracle.gen_golden.gen_cvt_variants; the fixture holds the fields of one entry of
nano_cvt_variants.pt, the case itself, and the gradients of the three relative-position tables in full (about two minutes of CPU)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as RL  # noqa: E402
from oracle.gen_golden import OUT, build_cvt_variant  # noqa: E402
from tests import golden_utils as GU  # noqa: E402

CASE = dict(cfg=dict(dims=(64, 128), heads=(1, 2), depths=(2, 1), rel_pos_embed=True, res_stem=True, windows=(14, 7)),
            sizes=(112, 64), n_local=2, B=2)


def main():
    ns = RL.load()
    RL.ensure_single_process_group()
    case = CASE
    student, teacher = build_cvt_variant(ns, case), build_cvt_variant(ns, case, teacher=True)
    GU.fill_state_dict(student.state_dict(), seed=0)
    GU.fill_state_dict(teacher.state_dict(), seed=7)
    for m in (student, teacher):
        for k, v in m.state_dict().items():
            if k.endswith("running_var"):
                v.abs_().add_(0.5)
    student.head.last_layer.weight_g.data.fill_(1)
    for p in teacher.parameters():
        p.requires_grad = False
    crops = GU.make_crops(case["B"], n_local=case["n_local"], sizes=case["sizes"])
    g = {"case": case,
         "keys": [(k, tuple(v.shape), str(v.dtype)) for k, v in student.state_dict().items()],
         "param_names": [n for n, _ in student.named_parameters()]}
    loss_fn = ns.DDINOLoss(GU.NANO_HEAD["out_dim"], 2 + case["n_local"], 0.04, 0.07, 5, 10)
    t_out = teacher(crops[:2])
    s_out = student(crops)
    for nm, t in (("s_cls", s_out[0]), ("s_reg", s_out[1]), ("s_fea", s_out[2]), ("t_cls", t_out[0]), ("t_reg", t_out[1]), ("t_fea", t_out[2])):
        g[nm] = GU.probe(t)
    g["npatch"] = (list(s_out[3]), list(t_out[3]))
    loss = loss_fn(s_out, t_out, 2, None)
    g["ddino_loss"] = loss.item()
    student.zero_grad()
    loss.backward()
    g["grads"] = {n: GU.probe(p.grad) for n, p in student.named_parameters() if p.grad is not None}
    g["grad_norms"] = {n: p.grad.norm().item() for n, p in student.named_parameters() if p.grad is not None}
    g["bn_buffers"] = {k: v.detach().clone() for k, v in student.state_dict().items() if "running_" in k or "num_batches" in k}
    g["table_grads"] = {n: p.grad.detach().clone() for n, p in student.named_parameters() if "rel_pos_bias_table" in n}
    assert sorted(tuple(t.shape) for t in g["table_grads"].values()) == [(169, 2), (729, 1), (729, 1)]
    torch.save(g, os.path.join(OUT, "nano_cvt_rpe_w14.pt"))
    print("nano_cvt_rpe_w14.pt: loss", g["ddino_loss"], "npatch", g["npatch"], "params", len(g["param_names"]),
          "table gradient norms", {n: "%.3e" % t.norm().item() for n, t in g["table_grads"].items()})


if __name__ == "__main__":
    main()
