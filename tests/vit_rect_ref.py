"""The fp64 statement of the position-grid resampling of a ViT on an (h, w) patch grid (esvit_amd.functional.vit_pos_resample; the
reference's forward_selfattention, models/vision_transformer.py:296-312), the bound its comparisons use, and mutants of it.

The statement.  The S x S grid of position vectors (S = int(sqrt(N))) goes through torch's F.interpolate(mode="bicubic") with the
scale-factor tuple (gh / sqrt(N), gw / sqrt(N)), each a Python double.  Per axis: floor(S * sf) output lines; line d reads the source
coordinate x = s (d + 0.5) - 0.5 with s the float32 value of 1 / sf (the kernel is handed the scale factor, not the size ratio;
align_corners False); the four taps floor(x) - 1 .. floor(x) + 2 carry the cubic-convolution weights with A = -0.75 and are clamped
to the border.  Where floor(S * sf) is short of the grid (side 61 from S = 14 or 28) the missing lines are zero: the reference's
`helper` padding (its second pad branch, for short columns, assigns to a name nobody reads and then fails; zero columns are what it
means).  All of it here in Python floats (fp64), tap by tap.

The bound, per output element, with u = 2^-24:
    B = 32 u sum|Ry||Rx||p| + 4 u S (sum|dRy||Rx||p| + sum|Ry||dRx||p|)
first term: the fp32 weights and a 16-term sum (<= 16 roundings of the products and the adds, twice over for the rounded weights and
the rounded intermediate of a separable evaluation); second term: one ulp of an fp32 source coordinate (x < S, so ulp(x) <= 2 u S, and
as much again for the rounding of s and of the product s (d + 0.5)), through the derivative dR of the weights with respect to the
coordinate.  The cubic convolution kernel is C1, so a coordinate that lands on the other side of an integer moves the result by the
same first-order amount.

The backward bound (gradient of the S x S grid for an upstream gradient g on the gh x gw grid), in the same form: element (a, b) sums
T(a, b) = nnz(Ry[:, a]) nnz(Rx[:, b]) products, where the forward sums 16, so
    Bg = 2 T u sum|Ry|^T|g||Rx| + 4 u S (sum|dRy|^T|g||Rx| + sum|Ry|^T|g||dRx|)."""
import math

import numpy as np
import torch

U = 2.0 ** -24
# S -> (gh, gw)
CASES = [(14, 6, 6), (14, 30, 45), (14, 3, 20), (14, 61, 2), (14, 2, 61), (14, 1, 1), (14, 14, 13), (4, 3, 5), (4, 2, 6), (28, 60, 80)]
MUTANTS = ("a_half", "align_corners", "size_ratio", "zero_taps", "swapped_axes", "replicate_last")


def cubic_weights(t, A=-0.75):
    """(weights of the taps -1, 0, 1, 2 at fraction t, their derivatives with respect to t)"""
    def far(z):
        return ((A * z - 5 * A) * z + 8 * A) * z - 4 * A, (3 * A * z - 10 * A) * z + 8 * A

    def near(z):
        return ((A + 2) * z - (A + 3)) * z * z + 1, (3 * (A + 2) * z - 2 * (A + 3)) * z
    w0, d0 = far(t + 1)
    w1, d1 = near(t)
    w2, d2 = near(1 - t)
    w3, d3 = far(2 - t)
    return (w0, w1, w2, w3), (d0, d1, -d2, -d3)


def n_lines(S, n_base, g):
    """lines the interpolation itself produces for g asked: floor(S * sf), sf = g / sqrt(n_base)"""
    return int(math.floor(S * (g / math.sqrt(n_base))))


def axis(S, g, mutant=None, n_base=None):
    """-> (R, dR) fp64 [g, S]: the axis matrix and its derivative with respect to the source coordinate"""
    n_base = S * S if n_base is None else n_base
    sf = g / math.sqrt(n_base)
    n_out = min(g, n_lines(S, n_base, g))
    s = float(np.float32(1.0 / sf))
    if mutant == "size_ratio":
        s = S / n_out
    R, dR = np.zeros((g, S)), np.zeros((g, S))
    for d in range(n_out):
        x = s * (d + 0.5) - 0.5
        if mutant == "align_corners":
            x = d * (S - 1) / (n_out - 1) if n_out > 1 else 0.0
        ix = math.floor(x)
        w, dw = cubic_weights(x - ix, -0.5 if mutant == "a_half" else -0.75)
        for k in range(4):
            j = ix - 1 + k
            if mutant == "zero_taps" and not 0 <= j < S:
                continue
            j = min(max(j, 0), S - 1)
            R[d, j] += w[k]
            dR[d, j] += dw[k]
    if mutant == "replicate_last":
        R[n_out:] = R[n_out - 1]
        dR[n_out:] = dR[n_out - 1]
    return R, dR


def grid_input(S, C=8, seed=0):
    """a deterministic S x S grid of C-vectors, fp32 values"""
    g = torch.Generator().manual_seed(1000 * S + seed)
    return torch.randn(S, S, C, generator=g)


def _apply(Ry, Rx, p):
    return np.einsum("ia,jb,abc->ijc", Ry, Rx, p)


def resample64(p, gh, gw, mutant=None):
    """p fp32 / fp64 [S, S, C] -> (value fp64 [gh, gw, C], bound B fp64 [gh, gw, C])"""
    p = p.double().numpy()
    S = p.shape[0]
    (Ry, dRy), (Rx, dRx) = axis(S, gh, mutant), axis(S, gw, mutant)
    if mutant == "swapped_axes":
        val = _apply(Ry, Rx, p.transpose(1, 0, 2))
    else:
        val = _apply(Ry, Rx, p)
    a = np.abs
    B = 32 * U * _apply(a(Ry), a(Rx), a(p)) + 4 * U * S * (_apply(a(dRy), a(Rx), a(p)) + _apply(a(Ry), a(dRx), a(p)))
    return torch.from_numpy(val), torch.from_numpy(B)


def resample_bwd64(g, S, gh, gw):
    """upstream gradient g [gh, gw, C] -> (gradient of the S x S grid fp64 [S, S, C], its bound Bg)"""
    g = g.double().numpy()
    (Ry, dRy), (Rx, dRx) = axis(S, gh), axis(S, gw)

    def adj(Y, X, t):
        return np.einsum("ia,jb,ijc->abc", Y, X, t)
    a = np.abs
    T = np.outer((Ry != 0).sum(0), (Rx != 0).sum(0))[:, :, None]
    Bg = 2 * T * U * adj(a(Ry), a(Rx), a(g)) + 4 * U * S * (adj(a(dRy), a(Rx), a(g)) + adj(a(Ry), a(dRx), a(g)))
    return torch.from_numpy(adj(Ry, Rx, g)), torch.from_numpy(Bg)


def torch_interpolate(p, gh, gw):
    """torch's own route: F.interpolate with the scale-factor tuple, then the zero lines -> fp32 / fp64 [gh, gw, C] (the dtype of p)"""
    S = p.shape[0]
    t = torch.nn.functional.interpolate(p.permute(2, 0, 1).unsqueeze(0), scale_factor=(gh / math.sqrt(S * S), gw / math.sqrt(S * S)), mode="bicubic")
    out = p.new_zeros(1, p.shape[2], gh, gw)
    out[:, :, :t.shape[2], :t.shape[3]] = t[:, :, :gh, :gw]
    return out[0].permute(1, 2, 0)


def worst_ratio(got, want, bound):
    """largest |got - want| / bound over the elements; an element with a zero bound must be exact"""
    err = (got.double() - want).abs()
    if ((bound == 0) & (err > 0)).any():
        return float("inf")
    return (err / bound.clamp_min(1e-300)).max().item()


# ---- tests/golden/vit_rect.pt (tools/gen_vit_rect_golden.py): the reference's VisionTransformer at the GU.NANO_VIT width on rectangles -------
# name: construction image size (base grid S = img / 16), batch, image (H, W) -> patch grid (H / 16, W / 16)
GOLD_CASES = {
    "s4_48x80": dict(img=64, B=2, H=48, W=80),      # 3 x 5
    "s4_32x96": dict(img=64, B=1, H=32, W=96),      # 2 x 6
    "s14_224x160": dict(img=224, B=1, H=224, W=160),  # 14 x 10
    "s14_976x32": dict(img=224, B=1, H=976, W=32),  # 61 x 2: 60 resampled rows and one zero row
}


def gold_images(name):
    c = GOLD_CASES[name]
    g = torch.Generator().manual_seed(sum(name.encode()))
    return torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
