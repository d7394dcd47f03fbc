"""Flip / rotation test-time augmentation on the HIP path (csrc/tta.hip).

``TTA(model, mode)`` wraps a model (or any callable [B,3,H,W] fp32 -> logits): one kernel writes the K
views of the batch (``unetseg_tta_views``), the model runs on the [K*B,3,H,W] batch, and one kernel
averages the class probabilities of the K outputs back in the identity frame and returns their log
(``unetseg_tta_merge``).  The result stands wherever logits do: its softmax is the mean probability,
so ``predict.predict_labels``, ``predict.predict_labels_tiled`` and the evaluation loops take the
wrapper in place of the model, unchanged.

View k in 0..7: f = k & 1, r = k >> 1; the W-flip (if f), then r counter-clockwise quarter turns,
``torch.rot90(torch.flip(x, [-1]) if f else x, r, (-2, -1))``.  A mode is an 8-bit mask of views
(``MODES``); a quarter turn (``d4``) needs a square input.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .lib import lib

#: mode name -> mask of views (bit k = view k)
MODES = {"none": 0x01, "hflip": 0x03, "flips": 0x33, "d4": 0xFF}
QUARTER_TURNS = 0xCC  # the views with odd r
MAX_CLASSES = 32


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def views(x, mask):
    """fp32 [K*B,C,H,W]: the views of x fp32 [B,C,H,W] named by ``mask``, view-major"""
    B, C, H, W = x.shape
    out = torch.empty(bin(mask).count("1") * B, C, H, W, dtype=torch.float32, device=x.device)
    lib.tta_views(x.data_ptr(), B, C, H, W, mask, out.data_ptr(), _stream(x))
    return out


def merge(logits, mask):
    """fp32 [B,C,H,W]: the log of the mean over the views of softmax(logits [K*B,C,H,W]) in the identity
    frame (C == 1: the logit of the mean sigmoid)"""
    K = bin(mask).count("1")
    N, C, H, W = logits.shape
    if N % K:
        raise ValueError(f"{N} outputs do not split into {K} views")
    if C > MAX_CLASSES:
        raise ValueError(f"the merge holds at most {MAX_CLASSES} classes, got C={C}")
    out = torch.empty(N // K, C, H, W, dtype=torch.float32, device=logits.device)
    lib.tta_merge(logits.data_ptr(), N // K, C, H, W, mask, out.data_ptr(), _stream(logits))
    return out


class TTA(nn.Module):
    """``model`` under the views of ``mode`` ("none", "hflip", "flips", "d4"); inference only.

    ``forward(x)``, x fp32 [B,3,H,W], returns what the model returns, merged over the views: a 4-D
    output [K*B,C,H,W] becomes [B,C,H,W] log mean probabilities (``unetseg_tta_merge``), a 2-D output
    [K*B,n] (classification logits) becomes log(mean_k softmax) in torch, and a tuple is merged member
    by member.  Outputs are converted with ``.float().contiguous()`` first, so bf16 autocast works.
    ``max_batch`` runs the K*B batch in consecutive chunks of at most that many images.
    ``mode="none"`` returns the model's own output untouched."""

    def __init__(self, model, mode="d4", max_batch=None):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"unknown TTA mode {mode!r} (one of {', '.join(MODES)})")
        if max_batch is not None and max_batch <= 0:
            raise ValueError(f"max_batch must be positive, got {max_batch}")
        self.model = model
        self.mode = mode
        self.mask = MODES[mode]
        self.max_batch = max_batch

    def _run(self, xv):
        if self.max_batch is None or xv.shape[0] <= self.max_batch:
            return self.model(xv)
        outs = [self.model(xv[i:i + self.max_batch]) for i in range(0, xv.shape[0], self.max_batch)]
        if isinstance(outs[0], (tuple, list)):
            return tuple(torch.cat([o[j] for o in outs]) for j in range(len(outs[0])))
        return torch.cat(outs)

    def _merge(self, o, n):
        if not torch.is_tensor(o) or o.shape[0] != n or o.dim() not in (2, 4):
            raise ValueError(f"cannot merge a model output of {tuple(o.shape) if torch.is_tensor(o) else type(o)} "
                             f"for {n} views x images")
        o = o.float().contiguous()
        if o.dim() == 4:
            return merge(o, self.mask)
        K = bin(self.mask).count("1")
        return torch.softmax(o.view(K, n // K, -1), -1).mean(0).log()

    def forward(self, x):
        if getattr(self.model, "training", False):
            raise RuntimeError("TTA is inference only: put the wrapped model in eval mode")
        if torch.is_grad_enabled():
            raise RuntimeError("TTA is inference only: call it under torch.no_grad()")
        if self.mode == "none":
            return self.model(x)
        if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError(f"TTA takes an fp32 [B,C,H,W] batch on the GPU, got {x.dtype} {tuple(x.shape)} "
                             f"on {x.device}")
        if self.mask & QUARTER_TURNS and x.shape[2] != x.shape[3]:
            raise ValueError(f"TTA mode {self.mode!r} turns the input by 90 degrees and needs H == W, got "
                             f"{x.shape[2]} x {x.shape[3]} (use 'flips')")
        xv = views(x.contiguous(), self.mask)
        out = self._run(xv)
        if isinstance(out, (tuple, list)):
            return tuple(self._merge(o, xv.shape[0]) for o in out)
        return self._merge(out, xv.shape[0])
