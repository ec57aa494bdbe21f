"""Bit-identity of the on-chip weight-gradient mode of esvit_mlp_fused_bwd between two library builds.  One process loads one library,
so each build writes the SHA-256 of every output at every row count, and a third call compares the two records:

    ESVIT_HIP_LIB=libA.so python tools/mlp_dw_identity.py dump a.json
    ESVIT_HIP_LIB=libB.so python tools/mlp_dw_identity.py dump b.json
    python tools/mlp_dw_identity.py compare a.json b.json

Row counts are those of tests/test_mlp_dw_moat_gpu.py (every branch of the tile walk) and one stage-0 row count of the training step;
each with and without DropPath row factors."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ("gx", "gxa", "dW2", "db2", "G", "db1")


def dump(path):
    import torch
    from esvit_amd import ops
    from esvit_amd._lib import LIB_PATH
    dev, C, dt = torch.device("cuda:0"), 96, torch.bfloat16
    G = ops.mlp_fused_dw_grid(dt, C, 1 << 40)
    g = torch.Generator().manual_seed(90)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    W1f, W2f = (r(4 * C, C) * 0.08).to(dev), (r(C, 4 * C) * 0.05).to(dev)
    gamma, beta, b1 = (1.0 + 0.2 * r(C)).to(dev), (0.1 * r(C)).to(dev), (0.1 * r(4 * C)).to(dev)
    K1, K2T, K1T = (ops.mlp_fused_weight(k, w) for k, w in ((ops.MLP_W1_BWD, W1f), (ops.MLP_W2T_BWD, W2f), (ops.MLP_W1T_BWD, W1f)))
    rec = dict(lib=os.path.basename(LIB_PATH), grid=G, cases={})
    for M in (1, 63, 64, 65, 64 * G + 1, 64 * 2 * G, 64 * 2 * G + 67, 128 * 576):
        gm = torch.Generator().manual_seed(91)
        x, gy = (torch.randn(M, C, generator=gm) * 1.5 + 0.3).to(dev), (torch.randn(M, C, generator=gm) * 0.5).to(dev)
        rm, ro = (torch.rand(M, generator=gm) > 0.3).float().div(0.7).to(dev), (torch.rand(M, generator=gm) > 0.2).float().div(0.8).to(dev)
        for dp in (False, True):
            outs = ops.mlp_fused_bwd_dw(x, gy, gamma, beta, 1e-6, K1, K2T, K1T, b1, rowscale_mlp=rm if dp else None, rowscale_out=ro if dp else None)
            torch.cuda.synchronize()
            rec["cases"]["M=%d droppath=%d" % (M, dp)] = {
                n: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() for n, t in zip(NAMES, outs)}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", path, "(%d cases, grid %d, %s)" % (len(rec["cases"]), G, rec["lib"]))


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    print("# SHA-256 of gx, gxa, dW2, db2, G, db1: %s against %s, %d workgroups" % (a["lib"], b["lib"], a["grid"]))
    assert a["grid"] == b["grid"] and a["cases"].keys() == b["cases"].keys()
    bad = 0
    for case, ha in a["cases"].items():
        diff = [n for n in NAMES if ha[n] != b["cases"][case][n]]
        bad += len(diff)
        print("%-28s %s" % (case, "identical (6 arrays)" if not diff else "DIFFERENT: " + ", ".join(diff)))
    print("arrays that differ: %d of %d" % (bad, 6 * len(a["cases"])))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
