"""The C-ABI calls of one step, in order, as text: the gate for a host-side refactor of the op layer.

    python tools/record_step_calls.py --model unet_resnet50 --dtype bf16 --batch 2 --size 256 --out FILE
        [--loss lovasz_hinge|bce] [--classes 5] [--eval] [--adam-overlap 0|1] [--warm 1]

Runs `--warm` eager steps (weights packed, query memo and workspaces warm), then one more step with a
logging wrapper installed the way StepPlan.record installs its own (lib._WRAP set, the lib caller's
cached attributes cleared, both restored afterwards).  One line per call: the entry point, the stream
it was issued on (s0, s1, ... by first appearance; `unetseg_stream_wait` also names the stream waited
for) and every argument -- a position that lib.SIGNATURES types as a pointer prints as 0 (null) or p,
everything else verbatim.  The last two lines are the step's count of Tensor.record_stream calls and
torch.cuda.max_memory_allocated() after it (peak reset before the logged step).  Two commits whose
files are equal issue the same launches with the same scalar arguments on the same streams, hand the
same number of tensors to the side stream and reach the same allocator peak; compare with cmp / sha256.
The environment switches (UNETSEG_NO_FUSE=1, ...) select the unfused branches as usual.

--eval logs one eval-mode forward under no_grad; --classes > 2 trains the multiclass head with CE + Dice
(the configuration of tests/test_gpu_round2.py::test_multiclass_head_model_fp32).
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402


class _CountRecordStream(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func._schema.name == "aten::record_stream":
            self.n += 1
        return func(*args, **(kwargs or {}))


class Log:
    def __init__(self):
        from unetseg_hip.lib import SIGNATURES
        self.sig = SIGNATURES
        self.lines = []
        self.streams = {}

    def _s(self, handle):
        return f"s{self.streams.setdefault(int(handle or 0), len(self.streams))}"

    def wrap(self, name, fn):
        argtypes = self.sig["unetseg_" + name][1]
        is_ptr = [t is ctypes.c_void_p for t in argtypes]

        def logged(*args):
            out = [name]
            if name == "stream_wait":
                out += [self._s(args[0]), "waits=" + self._s(args[1])]
            elif is_ptr and is_ptr[-1]:
                out.append(self._s(args[-1]))
            else:
                out.append("-")  # a host-only query (a memo miss)
            for a, ptr in zip(args, is_ptr):
                out.append(("p" if a else "0") if ptr else repr(a if not isinstance(a, int) else int(a)))
            self.lines.append(" ".join(out))
            return fn(*args)
        return logged


@contextlib.contextmanager
def logging_calls(log):
    """lib hands out log.wrap()ed callables and caches none (as StepPlan.record does)"""
    from unetseg_hip import lib as libmod
    saved = dict(libmod.lib.__dict__)
    libmod.lib.__dict__.clear()
    libmod._WRAP = log.wrap
    try:
        yield
    finally:
        libmod._WRAP = None
        libmod.lib.__dict__.clear()
        libmod.lib.__dict__.update(saved)


def build(args, dev):
    from model.model_factory import create_model
    from utils.synthetic import make_batch

    torch.manual_seed(11)
    multitask = args.model == "multitask_unet"
    kw = dict(num_classes=1) if multitask else dict(num_classes=args.classes)
    with contextlib.redirect_stdout(sys.stderr):
        model = create_model(args.model, weights="", **kw).to(dev)
    model.compute_dtype = args.dtype
    x, y, c = (t.to(dev) for t in make_batch(args.batch, args.size, seed=1234, with_cls=True))
    if args.eval:
        model.eval()

        def step():
            with torch.no_grad():
                return model(x)
        return step
    from unetseg_hip.arena import FusedAdam
    from unetseg_hip.losses import binary_segmentation_loss, multitask_loss
    model.train()
    opt = FusedAdam(model, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-4, overlap=bool(args.adam_overlap))
    if args.classes > 2:
        from model.unet_training import CE_Loss, Dice_loss
        C = args.classes
        g = torch.Generator().manual_seed(12)
        t = torch.randint(0, C + 1, (args.batch, args.size, args.size), generator=g)
        oh = torch.eye(C + 1)[t.reshape(-1)].reshape(args.batch, args.size, args.size, C + 1).to(dev)
        t, cw = t.to(dev), torch.ones(C, device=dev)
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if args.dtype == "bf16" else contextlib.nullcontext()

    def step():
        opt.zero_grad()
        with amp:
            if multitask:
                seg, cls = model(x)
                loss = multitask_loss(seg, cls, y, c, 1.0, args.loss)[0]
            elif args.classes > 2:
                out = model(x)
                loss = CE_Loss(out, t, cw, num_classes=C) + Dice_loss(out, oh)
            else:
                loss = binary_segmentation_loss(model(x), y, args.loss)
        loss.backward()
        opt.step()
        return loss
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="unet_resnet50")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--loss", default="lovasz_hinge")
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--adam-overlap", type=int, default=1)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    # a created stream, as in bench.py: its handle is not 0, so a 0 in a pointer position is a null pointer
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    step = build(args, dev)
    for _ in range(args.warm):
        step()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    log, count = Log(), _CountRecordStream()
    # autograd on this thread, so the backward's record_stream calls pass through the counting mode
    with torch.autograd.set_multithreading_enabled(False), logging_calls(log), count:
        step()
    torch.cuda.synchronize(dev)
    log.lines.append(f"# record_stream {count.n}")
    log.lines.append(f"# max_memory_allocated {torch.cuda.max_memory_allocated(dev)}")
    text = "\n".join(log.lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(f"{args.out}: {len(log.lines) - 2} calls, {log.lines[-2][2:]}, {log.lines[-1][2:]}, "
          f"sha256 {hashlib.sha256(text.encode()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
