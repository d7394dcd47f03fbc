"""CPU PyTorch restatement of the Lovasz-softmax loss (Berman, Rannen Triki, Blaschko, CVPR 2018,
Alg. 1, classes present in the segment, softmax errors), written from the paper's definition.  Helper
of test_gpu_lovasz_softmax.py / test_lovasz_softmax_cpu.py, not a test.

For one segment of pixels with p = softmax(logits) over the C classes, for every class c that occurs
among the segment's valid labels:
    fg_i = [label_i == c],  e_i = |fg_i - p_ic|  over the valid pixels, sorted descending
    J_k = 1 - (G - cumsum(fg)_k) / (G + cumsum(1 - fg)_k),  G = sum fg
    g_k = J_k - J_{k-1}  (J_0 = 0),   loss_c = sum_k e_(k) g_k
and the segment's loss is the mean of loss_c over the present classes, 0 without a valid pixel.
per_image: one segment per image, the loss is the mean over the B images (an image without a valid
pixel counts as 0); else one segment of all B * P pixels.  A pixel is invalid when its label equals
ignore_index or lies outside [0, C).  The sort is stable, so equal errors keep ascending pixel order;
autograd through the sorted dot product gives dL/de_(k) = g_k, the gradient the kernels implement.
"""
import torch


def lovasz_grad(fg_sorted):
    """g_k = J_k - J_{k-1} of the sorted 0/1 labels (Alg. 1, lines 3-9)"""
    G = fg_sorted.sum()
    inter = G - fg_sorted.cumsum(0)
    union = G + (1.0 - fg_sorted).cumsum(0)
    J = 1.0 - inter / union
    g = J.clone()
    g[1:] = J[1:] - J[:-1]
    return g


def _segment(probs, labels, ignore_index):
    """probs [C, N], labels [N] -> mean over the present classes of the class's Lovasz extension"""
    C = probs.shape[0]
    valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
    if not bool(valid.any()):
        return probs.sum() * 0.0
    pv, lv = probs[:, valid], labels[valid]
    per_class = []
    for c in range(C):
        fg = (lv == c).to(probs.dtype)
        if float(fg.sum()) == 0.0:
            continue
        err = (fg - pv[c]).abs()
        err_sorted, perm = torch.sort(err, descending=True, stable=True)
        per_class.append(torch.dot(err_sorted, lovasz_grad(fg[perm])))
    return torch.stack(per_class).mean()


def lovasz_softmax_ref(logits, labels, ignore_index, per_image=True, dtype=torch.float64):
    """logits [B, C, H, W] (a leaf that requires grad gets its gradient through autograd), labels
    [B, H, W]; every step runs in `dtype`"""
    x = logits.to(dtype)
    B, C = x.shape[0], x.shape[1]
    p = torch.softmax(x, dim=1).reshape(B, C, -1)
    lab = labels.reshape(B, -1)
    if per_image:
        return torch.stack([_segment(p[b], lab[b], ignore_index) for b in range(B)]).mean()
    return _segment(p.permute(1, 0, 2).reshape(C, -1), lab.reshape(-1), ignore_index)


def loss_and_grad(logits, labels, ignore_index, per_image=True, dtype=torch.float64):
    """(loss as a python float, d loss / d logits in float64) of the restatement run in `dtype`"""
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    loss = lovasz_softmax_ref(x, labels, ignore_index, per_image, dtype)
    if loss.requires_grad:
        loss.backward()
    g = x.grad if x.grad is not None else torch.zeros_like(x)
    return float(loss.detach()), g.double()
