"""Inference consumers of an EsViT checkpoint: the feature extraction and the weighted k-NN classifier
of the reference's eval_knn.py, on the HIP path.

``extract_features`` (eval_knn.py:165-190) runs the backbone (``build_model(config, is_teacher=True)`` with
``NUM_CLASSES 0``: the pooled cls features) batch by batch and gathers features and dataset indices of all ranks into
rank 0's feature matrix.  ``knn_classifier`` (eval_knn.py:193-232) scores every test feature against ALL train features
(cosine similarity of L2-normalised rows), keeps the k nearest, and lets them vote with weight exp(similarity / T).  The
similarity product -- the only heavy step: 50k x 1.28M x C for ImageNet -- is this library's fp32 MFMA GEMM reading the
train matrix in its stored [N_train, C] layout (no transposed copy); top-k, the one-hot vote and the ranking are
PyTorch indexing ops with the reference's tie behaviour.

``knn_classifier_multi`` is the fused route: ONE pass of ``ops.knn_topk`` at ``max(ks)`` -- similarity and
selection in one kernel, the [chunk, N_train] block never stored -- and a deterministic vote for every k from the prefix of the
sorted lists.  ``knn_topk_streamed`` scores a train matrix that arrives in pieces (host-resident features).  ``KNN_ROUTE``
(``ESVIT_KNN_ROUTE``) = "fused" sends ``knn_classifier`` through it; the default "gemm" is the per-k dense route.
"""
import os

import torch
import torch.distributed as dist

from . import ops


# which route knn_classifier takes: "gemm" (dense similarity block + torch.topk, once per k) or "fused" (knn_classifier_multi)
KNN_ROUTE = os.environ.get("ESVIT_KNN_ROUTE", "gemm")


def _dist_on():
    return dist.is_available() and dist.is_initialized()


def load_pretrained_weights(model, pretrained_weights, checkpoint_key, model_name=None, patch_size=None):
    """utils.load_pretrained_weights (utils.py:78-103): take `checkpoint_key` ("teacher" / "student") out of a training checkpoint
    written by main_esvit.py (utils.save_on_master), strip the DistributedDataParallel prefix, load non-strictly (the heads of the
    checkpoint have no place in a NUM_CLASSES 0 backbone).  Without a file the reference tries to download DINO's public ViT
    weights; there is no network on this side, so that branch leaves the random initialisation and says so.  Returns the
    load_state_dict message (the reference prints it)."""
    if not os.path.isfile(pretrained_weights):
        print("no checkpoint file at %r: the backbone keeps its random initialisation (the reference would fetch DINO's public weights "
              "here; this side has no network)" % (pretrained_weights,))
        return None
    ckpt = torch.load(pretrained_weights, map_location="cpu", weights_only=False)
    weights = ckpt.get(checkpoint_key, ckpt) if (checkpoint_key is not None and isinstance(ckpt, dict)) else ckpt
    if weights is not ckpt:
        print("checkpoint %s: using the %r entry" % (pretrained_weights, checkpoint_key))
    ddp_prefix = "module."  # utils.save_on_master stores the DistributedDataParallel-wrapped student
    weights = {(name[len(ddp_prefix):] if name.startswith(ddp_prefix) else name).replace("." + ddp_prefix, "."): tensor for name, tensor in weights.items()}
    report = model.load_state_dict(weights, strict=False)
    print("checkpoint %s loaded (non-strict): %s" % (pretrained_weights, report))
    return report


@torch.no_grad()
def extract_features(model, data_loader, use_cuda=True):
    """data_loader yields (samples, index) with ``index`` the position in ``data_loader.dataset`` (the reference's
    ReturnIndexDataset, eval_knn.py:235-238).  Returns the [len(dataset), C] feature matrix on rank 0, None elsewhere."""
    rank = dist.get_rank() if _dist_on() else 0
    world = dist.get_world_size() if _dist_on() else 1
    features = None
    dev = next(model.parameters()).device  # the reference hard-wires .cuda(); the model's device is the same thing on a GPU box
    for samples, index in data_loader:
        samples = samples.to(dev, non_blocking=True)
        index = index.to(dev, non_blocking=True)
        feats = model(samples).clone()
        if rank == 0 and features is None:
            features = torch.zeros(len(data_loader.dataset), feats.shape[-1])
            if use_cuda:
                features = features.to(dev, non_blocking=True)
        if world > 1:
            idx_l = [torch.empty_like(index) for _ in range(world)]
            dist.all_gather(idx_l, index)
            feat_l = [torch.empty_like(feats) for _ in range(world)]
            dist.all_gather(feat_l, feats)
            index_all, feats_all = torch.cat(idx_l), torch.cat(feat_l)
        else:
            index_all, feats_all = index, feats
        if rank == 0:
            if use_cuda:
                features.index_copy_(0, index_all, feats_all.float())
            else:
                features.index_copy_(0, index_all.cpu(), feats_all.float().cpu())
    return features


@torch.no_grad()
def knn_classifier(train_features, train_labels, test_features, test_labels, k, T, num_classes=1000, num_chunks=100):
    """-> (top1 %, top5 %).  Features are L2-normalised fp32 rows ([N_train, C], [N_test, C]) on the GPU.  The test set is
    scored in ``num_chunks`` chunks exactly as the reference does (eval_knn.py:197-198)."""
    if KNN_ROUTE == "fused":
        return knn_classifier_multi(train_features, train_labels, test_features, test_labels, (k,), T, num_classes=num_classes, num_chunks=num_chunks)[k]
    if KNN_ROUTE != "gemm":
        raise ValueError("esvit_amd.eval.KNN_ROUTE is %r: 'gemm' or 'fused'" % (KNN_ROUTE,))
    train_features = train_features.float().contiguous()
    test_features = test_features.float().contiguous()
    train_labels, test_labels = train_labels.to(train_features.device), test_labels.to(train_features.device)
    top1, top5, total = 0.0, 0.0, 0
    num_test = test_labels.shape[0]
    per_chunk = max(1, num_test // num_chunks)  # (the reference divides by 100 unguarded and fails below 100 test images)
    for idx in range(0, num_test, per_chunk):
        features = test_features[idx:min(idx + per_chunk, num_test)]
        targets = test_labels[idx:min(idx + per_chunk, num_test)]
        bs = targets.shape[0]
        similarity = ops.linear_fwd(features, train_features)  # [bs, N_train] = features @ train^T, fp32 MFMA GEMM
        distances, indices = similarity.topk(k, largest=True, sorted=True)
        neighbors = torch.gather(train_labels.view(1, -1).expand(bs, -1), 1, indices)
        one_hot = torch.zeros(bs * k, num_classes, device=similarity.device)
        one_hot.scatter_(1, neighbors.view(-1, 1), 1)
        weights = distances.clone().div_(T).exp_()
        probs = torch.sum(one_hot.view(bs, -1, num_classes) * weights.view(bs, -1, 1), 1)
        _, predictions = probs.sort(1, True)
        correct = predictions.eq(targets.view(-1, 1))
        top1 += correct.narrow(1, 0, 1).sum().item()
        top5 += correct.narrow(1, 0, min(5, num_classes)).sum().item()
        total += bs
    return top1 * 100.0 / total, top5 * 100.0 / total


# ------------------------------------------------------------------------------------------------------------------------
# the fused route: one top-k pass at max(ks), every k voted from its prefix
# ------------------------------------------------------------------------------------------------------------------------
def _topk_host(test, train, k, out=None, idx_base=0):
    """torch restatement of ops.knn_topk with its two orders (host tensors, or features the kernel does not take): larger
    similarity first, on equal similarities the smaller train row first (a STABLE descending sort over columns in row order).
    The similarity is accumulated in fp64 and rounded once, so that a column's value does not depend on the piece of the train
    matrix it arrived in -- what the kernel's fixed summation order gives on the GPU."""
    sim = (test.double() @ train.double().t()).float()
    cols = torch.arange(idx_base, idx_base + train.shape[0], dtype=torch.int32, device=sim.device).view(1, -1).expand(sim.shape[0], -1)
    if out is not None:  # the incoming lists hold earlier (smaller) row numbers: in front, so that the stable sort keeps them first on ties
        sim, cols = torch.cat([out[0], sim], 1), torch.cat([out[1], cols], 1)
    if k > sim.shape[1]:
        raise ValueError("knn_topk: k=%d exceeds the %d train rows" % (k, sim.shape[1]))
    vals, order = torch.sort(sim, dim=1, descending=True, stable=True)
    vals, idx = vals[:, :k].contiguous(), torch.gather(cols, 1, order[:, :k]).contiguous()
    if out is not None:
        out[0].copy_(vals)
        out[1].copy_(idx)
        return out
    return vals, idx


def _knn_topk(test, train, k, out=None, idx_base=0):
    if ops.knn_topk_supported(test, train):
        return ops.knn_topk(test.contiguous(), train.contiguous(), k, out=out, idx_base=idx_base)
    return _topk_host(test.float(), train.float(), k, out=out, idx_base=idx_base)


@torch.no_grad()
def knn_topk_streamed(test, train_chunks, k):
    """-> (vals [N_test, k], idx int32 [N_test, k]) of ``test`` against the concatenation of ``train_chunks`` (an iterable of
    [n_i, C] pieces, which may be host tensors: each is uploaded to the device of ``test``, scored and merged into the running
    lists, so the whole train matrix never has to be resident).  Equal, bit for bit, to the one-shot call on the concatenation.
    The first piece must hold at least k rows."""
    test = test.float().contiguous()
    out, base = None, 0
    for piece in train_chunks:
        piece = piece.to(test.device, non_blocking=True).float().contiguous()
        if piece.shape[0] == 0:
            continue
        if out is None and k > piece.shape[0]:
            raise ValueError("knn_topk_streamed: the first piece holds %d rows, fewer than k=%d" % (piece.shape[0], k))
        out = _knn_topk(test, piece, k, out=out, idx_base=base)
        base += piece.shape[0]
    if out is None:
        raise ValueError("knn_topk_streamed: no train rows")
    return out


def _vote(vals, labels, targets, ks, T, num_classes):
    """-> {k: (top-1 hits, top-5 hits)} of one chunk of test rows.  Class c collects exp(sim / T) of the neighbours labelled c, added
    one neighbour at a time in neighbour order (fp32; gather -> add -> scatter with one index per row: no atomics, deterministic),
    so the votes after k neighbours serve k.  The target's rank: classes with a strictly larger vote, plus classes with an equal
    vote and a smaller id."""
    rows = vals.shape[0]
    weights = vals.clone().div_(T).exp_()
    probs = torch.zeros(rows, num_classes, device=vals.device)
    class_id = torch.arange(num_classes, device=vals.device).view(1, -1)
    tcol = targets.view(-1, 1)
    hits, want = {}, set(ks)
    for j in range(max(ks)):
        lab = labels[:, j:j + 1]
        probs.scatter_(1, lab, probs.gather(1, lab) + weights[:, j:j + 1])
        if j + 1 in want:
            mine = probs.gather(1, tcol)
            rank = (probs > mine).sum(1) + ((probs == mine) & (class_id < tcol)).sum(1)
            hits[j + 1] = ((rank == 0).sum().item(), (rank < min(5, num_classes)).sum().item())
    return hits


@torch.no_grad()
def knn_classifier_multi(train_features, train_labels, test_features, test_labels, ks, T, num_classes=1000, num_chunks=100):
    """-> {k: (top1 %, top5 %)} for every k of ``ks`` from ONE neighbour search at max(ks): with a total order (larger similarity
    first, then the smaller train row) the k nearest are the first k of the max(ks) nearest.  On the GPU (fp32 features, C % 4 == 0)
    the search is ops.knn_topk; on host tensors its torch restatement.  The vote is chunked so that its scratch stays within the
    reference's own (N_test / num_chunks) * k * num_classes floats (eval_knn.py:199)."""
    ks = tuple(int(k) for k in ks)
    kmax = max(ks)
    if min(ks) < 1:
        raise ValueError("knn_classifier_multi: k must be positive")
    if kmax > train_features.shape[0]:
        raise ValueError("knn_classifier_multi: k=%d exceeds the %d train rows" % (kmax, train_features.shape[0]))
    train_features = train_features.float().contiguous()
    test_features = test_features.float().contiguous()
    dev = train_features.device
    train_labels, test_labels = train_labels.to(dev), test_labels.to(dev)
    num_test = test_labels.shape[0]
    if test_features.is_cuda and kmax > ops.KNN_MAX_K:  # (beyond the kernel's k: the restatement)
        vals, idx = _topk_host(test_features, train_features, kmax)
    else:
        vals, idx = _knn_topk(test_features, train_features, kmax)
    labels = train_labels[idx.long()]
    rows_per_vote = max(1, num_test // num_chunks) * kmax  # rows * num_classes floats <= the reference's rows * k * num_classes
    top = {k: [0, 0] for k in ks}
    for i in range(0, num_test, rows_per_vote):
        sl = slice(i, min(i + rows_per_vote, num_test))
        for k, (h1, h5) in _vote(vals[sl], labels[sl], test_labels[sl], ks, T, num_classes).items():
            top[k][0] += h1
            top[k][1] += h5
    return {k: (top[k][0] * 100.0 / num_test, top[k][1] * 100.0 / num_test) for k in ks}


# ------------------------------------------------------------------------------------------------------------------------
# eval_linear.py: the linear probe on frozen features (eval_linear.py:244-325)
# ------------------------------------------------------------------------------------------------------------------------
class _ProbeLinearFn(torch.autograd.Function):
    """y = x W^T + b on the library's fp32 MFMA GEMM (forward, data gradient is not needed -- the features are frozen --,
    weight gradient with the bias gradient fused)"""

    @staticmethod
    def forward(ctx, x, W, b):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.linear_fwd(x, W.detach().contiguous(), b.detach())

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        dW, db = ops.linear_wgrad(gy.contiguous(), x, want_bias=True)
        return None, dW, db


class LinearClassifier(torch.nn.Module):
    """eval_linear.py:307-321: one nn.Linear on the flattened frozen features, N(0, 0.01) weights, zero bias -- same module tree
    (``linear.weight`` / ``linear.bias``), so the reference's probe checkpoints (checkpoint.pth.tar: "state_dict") load"""

    def __init__(self, dim, num_labels=1000):
        super().__init__()
        self.linear = torch.nn.Linear(dim, num_labels)
        self.linear.weight.data.normal_(mean=0.0, std=0.01)
        self.linear.bias.data.zero_()

    def forward(self, x):
        x = x.view(x.size(0), -1)
        if x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0 and self.linear.out_features % 4 == 0:  # (the fp32 GEMM's 16-byte rows)
            return _ProbeLinearFn.apply(x, self.linear.weight, self.linear.bias)
        return self.linear(x)  # (host tensors: the CPU tests of the loop logic)


def accuracy(output, target, topk=(1,)):
    """utils.py:559-566"""
    maxk = max(topk)
    _, pred = output.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.reshape(1, -1).expand_as(pred.t()))
    return [correct[:k].reshape(-1).float().sum(0) * 100.0 / target.size(0) for k in topk]


def _features(model, inp, n, avgpool, depths):
    with torch.no_grad():
        return model.forward_return_n_last_blocks(inp, n, avgpool, depths).float()


def train_linear_epoch(model, linear_classifier, optimizer, loader, epoch, n, avgpool, depths):
    """eval_linear.train (eval_linear.py:244-277): frozen backbone features (forward_return_n_last_blocks, HIP path) -> linear
    classifier -> cross-entropy -> SGD step.  Returns the epoch means the reference logs ({"loss", "lr"}), rank-averaged."""
    linear_classifier.train()
    dev = next(linear_classifier.parameters()).device
    loss_sum, lr_sum, count = torch.zeros((), device=dev), 0.0, 0
    for inp, target in loader:
        inp, target = inp.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        output = linear_classifier(_features(model, inp, n, avgpool, depths))
        loss = torch.nn.functional.cross_entropy(output, target)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        loss_sum += loss.detach()
        lr_sum += optimizer.param_groups[0]["lr"]
        count += 1
    stats = torch.stack([loss_sum, torch.tensor(float(count), device=dev)])
    if _dist_on():
        dist.all_reduce(stats)
    return {"loss": (stats[0] / stats[1].clamp(min=1)).item(), "lr": lr_sum / max(count, 1)}


@torch.no_grad()
def validate_network(val_loader, model, linear_classifier, n, avgpool, depths):
    """eval_linear.validate_network (eval_linear.py:280-304) -> {"loss", "acc1", "acc5"}: loss averaged per batch, accuracies per
    sample, as the reference's MetricLogger does"""
    linear_classifier.eval()
    dev = next(linear_classifier.parameters()).device
    acc = torch.zeros(5, device=dev)  # sum of batch losses, batches, sum acc1 * bs, sum acc5 * bs, samples
    for inp, target in val_loader:
        inp, target = inp.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        output = linear_classifier(_features(model, inp, n, avgpool, depths))
        loss = torch.nn.functional.cross_entropy(output, target)
        a1, a5 = accuracy(output, target, topk=(1, min(5, output.shape[1])))
        bs = inp.shape[0]
        acc += torch.stack([loss, torch.ones((), device=dev), a1 * bs, a5 * bs, torch.tensor(float(bs), device=dev)])
    if _dist_on():
        dist.all_reduce(acc)
    return {"loss": (acc[0] / acc[1].clamp(min=1)).item(), "acc1": (acc[2] / acc[4].clamp(min=1)).item(), "acc5": (acc[3] / acc[4].clamp(min=1)).item()}


# the linear-probe sweep (esvit_amd/probe.py): every (learning rate, weight decay) of the probe from one frozen-feature pass
from .probe import LinearProbeSweep, train_linear_sweep_epoch, validate_linear_sweep  # noqa: E402,F401
