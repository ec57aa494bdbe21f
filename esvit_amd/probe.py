"""Linear-probe sweep: G linear classifiers -- one per (learning rate, weight decay) pair -- trained on ONE pass
of the frozen backbone per batch, instead of G runs of eval_linear.py that each repeat the backbone forward.

The members share the feature batch and differ only in their hyper-parameters, so the forward is one GEMM against the stacked weights
([B, D] x [G*C, D]^T), the weight / bias gradient is one GEMM ([G*C, B] x [B, D], bias gradient fused), and the two pieces that keep
the members apart are the library's: the class-index cross-entropy over the B*G rows of C logits (``ops.probe_ce``) and the per-member
SGD rule of the fused update (``ops.RULE_SGD_MEMBERS``: lr and wd per tensor from the table, the non-finite guard per member).
No member reads anything another member wrote: logit columns, gradient rows and update are disjoint, so member g is the stand-alone
``LinearClassifier`` + ``torch.optim.SGD`` run at its (lr, wd), and a member that diverges is frozen without touching the others.

On host tensors, in another dtype than fp32, or when ``num_labels`` / ``dim`` is not a multiple of 4 (the fp32 GEMM's 16-byte rows: the
gate of ``LinearClassifier.forward``) the same module runs the torch restatement below, member by member, in the module's dtype.
"""
import math

import numpy as np
import torch
import torch.distributed as dist

from . import ops

TFIELDS = 12  # columns of the fused update's tensor table (include/esvit_hip.h)


def _dist_on():
    return dist.is_available() and dist.is_initialized()


def _features(model, inp, n, avgpool, depths):
    with torch.no_grad():
        return model.forward_return_n_last_blocks(inp, n, avgpool, depths).float()


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def ce_rows_host(z, target):
    """torch restatement of ``ops.probe_ce`` in the dtype of ``z`` [B, G, C] with ``target`` [B] -> (row_loss [B, G, 2], softmax - onehot
    [B, G, C]).  row_loss[..., 0] = lse(z) - z_t; row_loss[..., 1] = #{j : z_j > z_t} + #{j < t : z_j == z_t}, the target's place in the
    stable descending order.  A row with a NaN / inf logit: loss NaN, rank C, NaN gradient."""
    B, G, C = z.shape
    t = target.long().view(B, 1, 1).expand(B, G, 1)
    zt = z.gather(2, t)
    loss = torch.logsumexp(z, 2) - zt[..., 0]
    col = torch.arange(C, device=z.device).view(1, 1, C)
    rank = ((z > zt) | ((z == zt) & (col < t))).sum(2)
    d = torch.softmax(z, 2)
    d.scatter_add_(2, t, torch.full_like(zt, -1.0))
    bad = ~torch.isfinite(z).all(2)
    loss = torch.where(bad, torch.full_like(loss, float("nan")), loss)
    rank = torch.where(bad, torch.full_like(rank, C), rank)
    d = torch.where(bad.unsqueeze(2), torch.full_like(d, float("nan")), d)
    return torch.stack([loss, rank.to(z.dtype)], 2), d


class LinearProbeSweep(torch.nn.Module):
    """G = len(lrs) * len(weight_decays) members, lr-major: member g = (lrs[g // len(weight_decays)], weight_decays[g % len(..)]).
    ``weight`` [G, num_labels, dim] and ``bias`` [G, num_labels] start as ONE N(0, 0.01) draw / zero replicated to every member
    (LinearClassifier's initialisation, eval_linear.py:312-313), the momentum buffers as zero.  ``lrs`` are the members' base learning
    rates, already scaled by the caller's batch * world / 256 rule; ``set_epoch`` applies the cosine schedule to them."""

    def __init__(self, dim, num_labels, lrs, weight_decays=(0.0,), momentum=0.9):
        super().__init__()
        lrs, weight_decays = [float(v) for v in lrs], [float(v) for v in weight_decays]
        if not lrs or not weight_decays:
            raise ValueError("LinearProbeSweep: at least one learning rate and one weight decay")
        self.dim, self.num_labels, self.momentum = int(dim), int(num_labels), float(momentum)
        self.base_lrs = [lr for lr in lrs for _ in weight_decays]
        self.member_wds = [wd for _ in lrs for wd in weight_decays]
        self.lrs = list(self.base_lrs)
        G = len(self.base_lrs)
        w0 = torch.empty(self.num_labels, self.dim).normal_(mean=0.0, std=0.01)
        self.weight = torch.nn.Parameter(w0.unsqueeze(0).repeat(G, 1, 1).contiguous(), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(G, self.num_labels), requires_grad=False)
        self.register_buffer("weight_momentum", torch.zeros(G, self.num_labels, self.dim))
        self.register_buffer("bias_momentum", torch.zeros(G, self.num_labels))
        # updates refused per member (a non-finite gradient statistic, and every update after the first refusal): counted where the
        # update runs, never read by the step
        self.register_buffer("skipped", torch.zeros(G, dtype=torch.int32))
        self._dev_state = None  # the kernel route's table, chunk list, gradient buffer (built on first use, rebuilt when lrs / storage change)

    # ---- hyper-parameters ------------------------------------------------------------------------------------------------------------
    @property
    def members(self):
        return len(self.base_lrs)

    @property
    def diverged(self):
        """bool [G] on the module's device: members frozen at their last finite values (no host synchronisation to read it there)"""
        return self.skipped > 0

    def set_lrs(self, lrs):
        lrs = [float(v) for v in lrs]
        if len(lrs) != self.members:
            raise ValueError("LinearProbeSweep.set_lrs: %d learning rates for %d members" % (len(lrs), self.members))
        self.lrs = lrs

    def set_epoch(self, epoch, epochs):
        """CosineAnnealingLR(T_max=epochs, eta_min=0) in closed form (eval_linear.py:191): lr_g = base_g (1 + cos(pi epoch / epochs)) / 2"""
        f = 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))
        self.set_lrs([b * f for b in self.base_lrs])

    def init_from(self, weight, bias=None):
        """every member starts from this [num_labels, dim] weight (and [num_labels] bias, default zero); momentum and counters are cleared"""
        with torch.no_grad():
            self.weight.copy_(weight.detach().to(self.weight).unsqueeze(0).expand_as(self.weight))
            if bias is None:
                self.bias.zero_()
            else:
                self.bias.copy_(bias.detach().to(self.bias).unsqueeze(0).expand_as(self.bias))
            self.weight_momentum.zero_()
            self.bias_momentum.zero_()
            self.skipped.zero_()

    def export(self, g):
        """member g as a LinearClassifier / reference probe checkpoint ("state_dict") entry"""
        return {"linear.weight": self.weight[g].detach().clone(), "linear.bias": self.bias[g].detach().clone()}

    def get_extra_state(self):
        return {"base_lrs": list(self.base_lrs), "weight_decays": list(self.member_wds), "lrs": list(self.lrs), "momentum": self.momentum}

    def set_extra_state(self, state):
        if len(state["base_lrs"]) != self.members:
            raise ValueError("LinearProbeSweep: checkpoint of %d members, module of %d" % (len(state["base_lrs"]), self.members))
        self.base_lrs, self.member_wds = [float(v) for v in state["base_lrs"]], [float(v) for v in state["weight_decays"]]
        self.lrs, self.momentum = [float(v) for v in state["lrs"]], float(state["momentum"])

    # ---- routes ----------------------------------------------------------------------------------------------------------------------
    def kernel_route(self, feats):
        return (feats.is_cuda and self.weight.is_cuda and self.weight.dtype == torch.float32 and self.dim % 4 == 0 and self.num_labels % 4 == 0)

    def logits(self, feats):
        """-> [B, G, C] logits of every member"""
        feats = feats.reshape(feats.shape[0], -1)
        G, C, D = self.weight.shape
        if self.kernel_route(feats):
            return ops.linear_fwd(feats.float().contiguous(), self.weight.view(G * C, D), self.bias.view(G * C), out_f32=True).view(-1, G, C)
        feats = feats.to(self.weight.dtype)
        # member by member: a member's numbers must not depend on how many others there are (a BLAS may block by the output width)
        return torch.stack([torch.addmm(self.bias[g], feats, self.weight[g].t()) for g in range(G)], 1)

    def _device_state(self, B, world):
        G, C, D = self.weight.shape
        key = (self.weight.data_ptr(), self.bias.data_ptr(), self.weight_momentum.data_ptr(), self.bias_momentum.data_ptr(), tuple(self.lrs),
               tuple(self.member_wds))
        st = self._dev_state
        if st is None or st["key"] != key:
            dev = self.weight.device
            grad = st["grad"] if st is not None and st["grad"].device == dev else torch.zeros(G * C * D + G * C, dtype=torch.float32, device=dev)
            gW, gb = grad[:G * C * D].view(G * C, D), grad[G * C * D:]
            tab = np.zeros((2 * G, TFIELDS), dtype=np.int64)
            chunk, chunks = ops.update_chunk_elems(), []
            for g in range(G):
                hyper = _bits(self.lrs[g]) | (_bits(self.member_wds[g]) << 32)
                hyper -= (1 << 64) if hyper >= 1 << 63 else 0
                rows = ((self.weight[g], gW[g * C:(g + 1) * C], self.weight_momentum[g]), (self.bias[g], gb[g * C:(g + 1) * C], self.bias_momentum[g]))
                for k, (p, gr, mu) in enumerate(rows):
                    i = 2 * g + k
                    tab[i, 0], tab[i, 1], tab[i, 2], tab[i, 5] = p.data_ptr(), gr.data_ptr(), mu.data_ptr(), p.numel()
                    tab[i, 7], tab[i, 9] = 1 | (g << 32), hyper
                    chunks.extend((i, ci) for ci in range(-(-p.numel() // chunk)))
            st = dict(key=key, grad=grad, gW=gW, gb=gb, table=torch.from_numpy(tab).to(dev), nchunks=len(chunks),
                      chunks=torch.tensor(chunks, dtype=torch.int32).to(dev), sqnorms=torch.zeros(2 * G, dtype=torch.float32, device=dev), row_w={})
            self._dev_state = st
        if (B, world) not in st["row_w"]:
            st["row_w"][(B, world)] = torch.full((B * G,), 1.0 / (B * world), dtype=torch.float32, device=self.weight.device)
        return st

    @torch.no_grad()
    def step(self, feats, target):
        """one SGD step of every member on the feature batch -> the members' batch-mean losses [G] (on the device, before the step).
        Under torch.distributed the gradients of all members -- one flat buffer, scaled by 1 / (B * world) -- are all-reduced once."""
        feats = feats.reshape(feats.shape[0], -1)
        B = feats.shape[0]
        G, C, D = self.weight.shape
        world = dist.get_world_size() if _dist_on() else 1
        if self.kernel_route(feats):
            feats = feats.float().contiguous()
            st = self._device_state(B, world)
            logits = ops.linear_fwd(feats, self.weight.view(G * C, D), self.bias.view(G * C), out_f32=True)
            tgt = target.to(torch.int32).view(B, 1).expand(B, G).contiguous().view(-1)
            row_loss, dlogits = ops.probe_ce(logits.view(B * G, C), tgt, st["row_w"][(B, world)])  # in place: the logits become their gradient
            ops.linear_wgrad(dlogits.view(B, G * C), feats, want_bias=True, out=st["gW"], db_out=st["gb"])
            if world > 1:
                dist.all_reduce(st["grad"])
            ops.grad_sqnorm(st["table"], 2 * G, st["chunks"], st["nchunks"], st["sqnorms"], stats=1)
            ops.fused_clip_update_ema(ops.RULE_SGD_MEMBERS, st["table"], 2 * G, st["chunks"], st["nchunks"], st["sqnorms"], 0.0, 0.0, 0.0,
                                      self.momentum, 0.0, 0.0, 0.0, skipped=self.skipped)
            return row_loss.view(B, G, 2)[:, :, 0].sum(0) / B
        return self._step_host(feats.to(self.weight.dtype), target, world)

    def _step_host(self, feats, target, world):
        B = feats.shape[0]
        G, C, D = self.weight.shape
        dt, dev = self.weight.dtype, self.weight.device
        row_loss, d = ce_rows_host(self.logits(feats), target)
        d = d * (1.0 / (B * world))
        grad = torch.empty(G * C * D + G * C, dtype=dt, device=dev)
        gW, gb = grad[:G * C * D].view(G, C, D), grad[G * C * D:].view(G, C)
        for g in range(G):  # (member by member, as in logits())
            torch.mm(d[:, g].t(), feats, out=gW[g])
        torch.sum(d, 0, out=gb)
        if world > 1:
            dist.all_reduce(grad)
        # the per-member guard of ESVIT_RULE_SGD_MEMBERS on the statistics of esvit_grad_sqnorm: sum g^2 of the weight, of the bias
        bad = ~torch.isfinite((gW * gW).sum((1, 2))) | ~torch.isfinite((gb * gb).sum(1)) | (self.skipped > 0)
        self.skipped += bad.to(torch.int32)
        lr = torch.tensor(self.lrs, dtype=dt, device=dev)
        wd = torch.tensor(self.member_wds, dtype=dt, device=dev)
        for p, gr, mu, shape in ((self.weight, gW, self.weight_momentum, (G, 1, 1)), (self.bias, gb, self.bias_momentum, (G, 1))):
            keep = bad.view(shape)
            mu_new = self.momentum * mu + (gr + wd.view(shape) * p)
            p.copy_(torch.where(keep, p, p - lr.view(shape) * mu_new))
            mu.copy_(torch.where(keep, mu, mu_new))
        return row_loss[:, :, 0].sum(0) / B

    @torch.no_grad()
    def evaluate(self, feats, target):
        """-> (batch-mean loss [G], top-1 hits [G], top-min(5, C) hits [G]) of every member on the feature batch, on the device"""
        feats = feats.reshape(feats.shape[0], -1)
        B = feats.shape[0]
        G, C, D = self.weight.shape
        if self.kernel_route(feats):
            logits = ops.linear_fwd(feats.float().contiguous(), self.weight.view(G * C, D), self.bias.view(G * C), out_f32=True)
            tgt = target.to(torch.int32).view(B, 1).expand(B, G).contiguous().view(-1)
            row_loss = ops.probe_ce(logits.view(B * G, C), tgt, None, want_grad=False)[0].view(B, G, 2)
        else:
            row_loss = ce_rows_host(self.logits(feats), target)[0]
        rank = row_loss[:, :, 1]
        return row_loss[:, :, 0].sum(0) / B, (rank < 1).sum(0), (rank < min(5, C)).sum(0)


def train_linear_sweep_epoch(model, sweep, loader, epoch, n, avgpool, depths):
    """eval_linear.train (eval_linear.py:244-277) for every member of ``sweep`` on one backbone forward per batch.  Returns a list of G
    {"loss", "lr"}: the loss averaged per batch, then over the ranks -- ``train_linear_epoch`` per member.  The per-member sums stay on
    the device until the epoch ends (one read)."""
    sweep.train()
    dev = sweep.weight.device
    G = sweep.members
    loss_sum, count = torch.zeros(G, dtype=sweep.weight.dtype, device=dev), 0
    for inp, target in loader:
        inp, target = inp.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        loss_sum += sweep.step(_features(model, inp, n, avgpool, depths), target)
        count += 1
    stats = torch.cat([loss_sum.double(), torch.tensor([float(count)], dtype=torch.float64, device=dev)])
    if _dist_on():
        dist.all_reduce(stats)
    stats = stats.tolist()
    return [{"loss": stats[g] / max(stats[G], 1.0), "lr": sweep.lrs[g]} for g in range(G)]


@torch.no_grad()
def validate_linear_sweep(val_loader, model, sweep, n, avgpool, depths):
    """eval_linear.validate_network (eval_linear.py:280-304) for every member -> (list of G {"loss", "acc1", "acc5"}, best_index): loss
    averaged per batch, accuracies per sample with min(5, C); a hit is the target's rank in the stable descending order of the logits
    (larger first, on equal logits the smaller class first) being below k.  best_index: the first member with the largest acc1."""
    sweep.eval()
    dev = sweep.weight.device
    G = sweep.members
    acc = torch.zeros(3 * G + 2, dtype=torch.float64, device=dev)  # per member: sum of batch losses, top-1 hits, top-5 hits; batches, samples
    for inp, target in val_loader:
        inp, target = inp.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        loss, h1, h5 = sweep.evaluate(_features(model, inp, n, avgpool, depths), target)
        acc[:G] += loss.double()
        acc[G:2 * G] += h1.double()
        acc[2 * G:3 * G] += h5.double()
        acc[3 * G] += 1.0
        acc[3 * G + 1] += float(inp.shape[0])
    if _dist_on():
        dist.all_reduce(acc)
    acc = acc.tolist()
    batches, samples = max(acc[3 * G], 1.0), max(acc[3 * G + 1], 1.0)
    out = [{"loss": acc[g] / batches, "acc1": acc[G + g] * 100.0 / samples, "acc5": acc[2 * G + g] * 100.0 / samples} for g in range(G)]
    best = max(range(G), key=lambda g: (out[g]["acc1"], -g))
    return out, best
