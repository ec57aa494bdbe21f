"""Training-health monitor of the DINO / EsViT losses: what the loss value cannot tell ("Training-health monitor").

The loss of a 65536-way self-distillation sits near ln K for a fresh network, for a teacher collapsed to the uniform distribution
and, up to the centre, for a teacher collapsed onto one prototype.  What tells these apart is the teacher's entropy per row (-> ln K
in a uniform collapse), the entropy of the batch-mean teacher distribution (-> 0 when one dimension dominates) and
KL(teacher || student) = CE - H(teacher), the quantity that really falls while learning; for the region task, how well and how widely
the argmax matching lands.

    loss.monitor = TrainingMonitor(period=10)        # on a DINOLoss / DDINOLoss; or the environment variable ESVIT_MONITOR=<period>

``loss.forward`` calls ``observe`` on due steps with what it already holds (logits, centres, row statistics, match tables, row
losses, the similarity tensor).  ``observe`` enqueues on the current stream -- one streaming kernel per level (ops.dist_stats) plus a
few small torch launches -- and adds into fp64 accumulators on the device: no .item(), no host decision on device values.
``compute()`` synchronises once and returns the means over the observed steps; engine.train_one_epoch calls it at the look it takes
every 10 iterations anyway.  The view level uses the bare key, the region level the suffix ``_grid``.
"""
import os

import torch


def dist_stats_torch(x, center, inv_temp, stats):
    """ops.dist_stats in fp32 torch, for an ops module without that entry (the CPU restatement): the same formulas and the same NaN rule"""
    mx, lse = stats
    y = x.float()
    if center is not None:
        y = y - center.view(1, -1)
    d = y * inv_temp - mx[:, None]
    p = torch.exp(d - lse[:, None])
    ent = lse - (p * d).sum(1)
    bad = ~(torch.isfinite(ent) & torch.isfinite(mx))
    ent = torch.where(bad, torch.full_like(ent, float("nan")), ent)
    amax = torch.where(bad, torch.full_like(mx, -1.0), y.argmax(1).float()).to(torch.int32)
    psum = p.sum(0)
    psum = torch.where(bad.any(), torch.full_like(psum, float("nan")), psum)
    return ent, amax, psum


def env_period():
    """ESVIT_MONITOR=<period>: a positive integer, anything else raises; unset or empty: no monitor"""
    v = os.environ.get("ESVIT_MONITOR", "")
    if v == "":
        return None
    if not (v.isascii() and v.isdigit() and int(v) > 0):
        raise ValueError("ESVIT_MONITOR: a positive integer (the period in steps), not %r" % v)
    return int(v)


def from_env():
    p = env_period()
    return None if p is None else TrainingMonitor(period=p)


def _entropy(p):
    return -torch.xlogy(p, p).sum()


class TrainingMonitor:
    """period: every period-th forward of the loss is observed (the first one included).  student=True adds ``student_entropy``: a
    second read of the student rows (180 per image), off by default."""

    def __init__(self, period=10, student=False):
        if not (isinstance(period, int) and period > 0):
            raise ValueError("TrainingMonitor: period is a positive integer, not %r" % (period,))
        self.period, self.student = period, bool(student)
        self._calls = 0
        self.reset()

    # ---- schedule ---------------------------------------------------------------------------------------------------------------
    def due(self):
        """called once per forward of the loss: True on forwards 0, period, 2 period, ..."""
        due = self._calls % self.period == 0
        self._calls += 1
        return due

    def reset(self):
        self._keys, self._acc, self._n = [], None, 0

    @property
    def observed(self):
        return self._n

    # ---- one level --------------------------------------------------------------------------------------------------------------
    def _level(self, o, out, sfx, t, center, inv_tt, t_stats, s, inv_st, s_stats, tmatch, weights, row_loss):
        dist = getattr(o, "dist_stats", None) or dist_stats_torch
        mx, lse = t_stats
        ent, amax, psum = dist(t, center.view(-1), inv_tt, (mx, lse))
        R = t.shape[0]
        out["teacher_entropy" + sfx] = ent.mean()
        out["teacher_marginal_entropy" + sfx] = _entropy(psum / R)
        out["teacher_pmax" + sfx] = torch.exp(-lse).mean()
        # KL(teacher || student) = CE - H(teacher): row_loss[r] = sum over the row's live terms of w CE
        tm = tmatch.view(row_loss.shape[0], -1).long()
        live = tm >= 0
        w = weights.view(-1, 1).expand_as(tm) if weights.numel() == tm.shape[0] else weights.view(tm.shape)
        w = torch.where(live, w, torch.zeros_like(w)).double()
        h = ent.double()[tm.clamp(min=0)]
        h = torch.where(live, h, torch.zeros_like(h))
        out["kl" + sfx] = (row_loss.double().sum() - (w * h).sum()) / w.sum()
        out["center_absmax" + sfx] = center.abs().max()
        if self.student:
            if s_stats is None:
                s_stats = o.teacher_row_stats(s, torch.zeros(s.shape[1], dtype=torch.float32, device=s.device), inv_st)
            out["student_entropy" + sfx] = dist(s, None, inv_st, s_stats)[0].mean()
        return amax

    @torch.no_grad()
    def observe(self, o, view, grid=None):
        """o: the ops module of the loss.  view / grid: dicts of one level's tensors -- t, center, inv_tt, t_stats, s, inv_st, s_stats,
        tmatch, weights, row_loss; the view level adds B (images), the region level sim [B, S, ld], Tt, crop_id [S], cm_row [B S] and
        ncrops."""
        out = {}
        lv = {k: view[k] for k in ("t", "center", "inv_tt", "t_stats", "s", "inv_st", "s_stats", "tmatch", "weights", "row_loss")}
        amax = self._level(o, out, "", **lv)
        B = view["B"]
        out["view_agreement"] = (amax[:B] == amax[B:2 * B]).double().mean()
        if grid is not None:
            lv = {k: grid[k] for k in ("t", "center", "inv_tt", "t_stats", "s", "inv_st", "s_stats", "tmatch", "weights", "row_loss")}
            self._level(o, out, "_grid", **lv)
            out["match_similarity"], out["match_coverage"] = match_stats(grid["sim"], grid["tmatch"], grid["Tt"], grid["crop_id"],
                                                                         grid["cm_row"], grid["ncrops"])
        keys = list(out)
        vals = torch.stack([out[k].double().reshape(()) for k in keys])
        if self._acc is None:
            self._keys, self._acc = keys, torch.zeros_like(vals)
        assert keys == self._keys, "TrainingMonitor: the observed quantities changed between steps (reset() first)"
        self._acc += vals
        self._n += 1

    def compute(self):
        """the means over the steps observed since reset(): one synchronisation; {} before the first observation"""
        if self._n == 0:
            return {}
        return dict(zip(self._keys, (self._acc / self._n).tolist()))


def match_stats(sim, tmatch, Tt, crop_id, cm_row, ncrops):
    """-> (mean winning cosine similarity over the live (student token, teacher view) pairs, mean share of the Tt teacher tokens of a
    view that are the match of at least one token of a student crop, over the (image, crop, view != crop) triples)"""
    B, S, _ = sim.shape
    dev = sim.device
    tm = tmatch.view(-1, 2)[cm_row.long()].view(B, S, 2).long()          # image-major
    live = tm >= 0
    base = (torch.arange(2, device=dev).view(1, 1, 2) * B + torch.arange(B, device=dev).view(B, 1, 1)) * Tt
    j = torch.where(live, tm - base, torch.zeros_like(tm))             # token within the view
    win = sim.gather(2, j + torch.arange(2, device=dev).view(1, 1, 2) * Tt)
    nlive = live.double().sum()
    similarity = torch.where(live, win, torch.zeros_like(win)).double().sum() / nlive
    hit = torch.zeros((B, ncrops, 2, Tt + 1), dtype=torch.float64, device=dev)  # (slot Tt takes the dead pairs)
    crop = crop_id.long().view(1, S, 1).expand(B, S, 2)
    bb = torch.arange(B, device=dev).view(B, 1, 1).expand(B, S, 2)
    qq = torch.arange(2, device=dev).view(1, 1, 2).expand(B, S, 2)
    hit.index_put_((bb, crop, qq, torch.where(live, j, torch.full_like(j, Tt))), torch.ones((), dtype=torch.float64, device=dev))
    pairs = B * (2 * ncrops - 2)                                       # every crop against the views that are not its own
    coverage = hit[..., :Tt].sum() / (pairs * Tt)
    return similarity, coverage
