"""Torch restatement of the fused k-NN scoring (esvit_gemm_desc::topk, esvit_amd.eval.knn_classifier_multi) that the tests compare
against: the one-shot top-k under the total order (larger similarity first, on equal similarities the smaller train row first) and
the vote with its rank rule, written independently of the package's own host branch."""
import torch


def topk_of(sim, k):
    """-> (vals [R, k], idx int32 [R, k]) of a similarity block: stable descending sort over columns in row-number order"""
    vals, order = torch.sort(sim, dim=1, descending=True, stable=True)
    return vals[:, :k].contiguous(), order[:, :k].to(torch.int32).contiguous()


def similarity_host(test, train):
    """fp64 product rounded once to fp32: a column's value does not depend on what else is in the train matrix"""
    return (test.double() @ train.double().t()).float()


def topk_host(test, train, k):
    return topk_of(similarity_host(test, train), k)


def vote(vals, idx, train_labels, test_labels, k, T, num_classes):
    """-> (top1 %, top5 %) from sorted neighbour lists: per row, class c gets the sum over the first k neighbours labelled c of
    exp(sim / T), added in neighbour order in fp32; the target's rank = classes with a strictly larger vote + classes with an
    equal vote and a smaller id"""
    rows = vals.shape[0]
    w = (vals[:, :k].clone() / T).exp()
    lab = train_labels[idx[:, :k].long()]
    top1 = top5 = 0
    for r in range(rows):
        probs = torch.zeros(num_classes)
        for j in range(k):
            probs[lab[r, j]] = probs[lab[r, j]] + w[r, j]
        t = int(test_labels[r])
        rank = int((probs > probs[t]).sum()) + int((probs[:t] == probs[t]).sum())
        top1 += rank == 0
        top5 += rank < min(5, num_classes)
    return top1 * 100.0 / rows, top5 * 100.0 / rows
