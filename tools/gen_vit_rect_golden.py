"""Generate tests/golden/vit_rect.pt from the REFERENCE's own VisionTransformer (needs the reference tree, oracle/ref_loader.py):

    python tools/gen_vit_rect_golden.py

Two models of the GU.NANO_VIT width (embed 64, depth 2, 2 heads, patch 16), built for 64^2 (base grid 4 x 4) and for 224^2 (14 x 14),
both filled with GU.fill_state_dict(..., 0), on the rectangular images of tests/vit_rect_ref.GOLD_CASES.  Per image the fixture holds
    attn1      forward_selfattention(x, 1)               [B, 2, N, N]
    attn2_0    forward_selfattention(x, 2)[0]            (its second entry is checked here to equal attn1 bit for bit, and not stored twice)
    feats      the output of the last block, as a forward hook on it sees it during forward_selfattention(x, 2)'s own token path, through
               the reference's final norm                [B, N, 64]
976 x 32 (grid 61 x 2) takes the reference's zero-row padding.  The mirrored 32 x 976 fails inside the reference (its second pad
branch) and has no entry: the fp64 statement of tests/vit_rect_ref.py pins it."""
import importlib
import os
import sys
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as RL  # noqa: E402
from tests import golden_utils as GU  # noqa: E402
from tests import vit_rect_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vit_rect.pt")


def build(img):
    vits = importlib.import_module("models.vision_transformer")  # the reference's module
    v = GU.NANO_VIT
    m = vits.VisionTransformer(img_size=[img], patch_size=v["patch"], embed_dim=v["embed_dim"], depth=v["depth"], num_heads=v["heads"],
                               mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), drop_path_rate=0.0)
    GU.fill_state_dict(m.state_dict(), 0)
    return m.eval()


def main():
    RL.load()
    models, out = {}, {}
    for name, c in R.GOLD_CASES.items():
        m = models.get(c["img"]) or models.setdefault(c["img"], build(c["img"]))
        x = R.gold_images(name)
        seen = {}
        # the last block's input on the route under test (patch embedding + the (w0, h0) position grid + the blocks before it)
        h = m.blocks[-1].register_forward_pre_hook(lambda mod, args, seen=seen: seen.__setitem__("x", args[0].detach().clone()))
        with torch.no_grad():
            a1 = m.forward_selfattention(x, 1)
            h.remove()
            a2 = m.forward_selfattention(x, 2)
            cap = {}
            h = m.blocks[-1].register_forward_hook(lambda mod, args, res, cap=cap: cap.__setitem__("y", res.detach().clone()))
            m.blocks[-1](seen["x"])
            h.remove()
            feats = m.norm(cap["y"])
        assert len(a2) == 2 and torch.equal(a2[1], a1)
        N = 1 + (c["H"] // 16) * (c["W"] // 16)
        assert a1.shape == (c["B"], 2, N, N) and feats.shape == (c["B"], N, 64)
        out[name] = dict(case=dict(c), attn1=a1.clone(), attn2_0=a2[0].clone(), feats=feats.clone())
        print(name, "tokens", N, "attn1 sum %.6f" % a1.double().sum().item(), "feats |.| %.6f" % feats.double().abs().mean().item())
    torch.save(out, OUT)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
