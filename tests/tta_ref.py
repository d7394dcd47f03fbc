"""torch / float64 restatement of the test-time-augmentation views and their merge (csrc/tta.hip,
unetseg_hip/tta.py), from torch.flip and torch.rot90 alone: no index arithmetic of the kernels' kind.

View k in 0..7: f = k & 1, r = k >> 1: the W-flip (if f), then r counter-clockwise quarter turns.  A
set of views is an 8-bit mask (bit k = view k), ordered by ascending k.
"""
import torch

FLT_MIN = 1.1754943508222875e-38


def ks(mask):
    return [k for k in range(8) if mask >> k & 1]


def view(x, k):
    """view k of x[..., H, W]"""
    f, r = k & 1, k >> 1
    return torch.rot90(torch.flip(x, dims=[-1]) if f else x, r, dims=(-2, -1))


def inverse(v, k):
    """undoes view(., k): back through the quarter turns, then the flip"""
    f, r = k & 1, k >> 1
    x = torch.rot90(v, -r, dims=(-2, -1))
    return torch.flip(x, dims=[-1]) if f else x


def views_ref(x, mask):
    """[K*B, C, H, W]: the views of x [B, C, H, W], view-major (x's dtype, a pure permutation)"""
    return torch.cat([view(x, k) for k in ks(mask)], 0).contiguous()


def merge_ref(logits, mask):
    """float64 [B, C, H, W] from logits [K*B, C, H, W] (slab k in view k's frame): the log of the mean
    over the views of the softmax over C, each slab first brought back to the identity frame; C == 1:
    log(mean sigmoid(z)) - log(mean sigmoid(-z)), each mean floored at FLT_MIN"""
    kk = ks(mask)
    K = len(kk)
    z = logits.detach().double().cpu()
    N, C = z.shape[:2]
    assert N % K == 0
    slabs = [inverse(s, k) for s, k in zip(z.view(K, N // K, *z.shape[1:]), kk)]
    if C == 1:
        p = torch.stack([torch.sigmoid(s) for s in slabs]).mean(0)
        q = torch.stack([torch.sigmoid(-s) for s in slabs]).mean(0)
        return p.clamp_min(FLT_MIN).log() - q.clamp_min(FLT_MIN).log()
    return torch.stack([torch.softmax(s, 1) for s in slabs]).mean(0).log()
