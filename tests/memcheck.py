"""Poisoned allocations with guard bands (a test helper, imported like tests_helpers.py).

``with Poison(0xFF) as mc:`` replaces ``torch.empty``, ``torch.zeros``, ``torch.empty_like``,
``torch.zeros_like``, ``Tensor.new_empty`` and ``Tensor.new_zeros`` for the duration of the block.
An allocation on the watched device (``cuda`` unless told otherwise) becomes a slice of one uint8
block of GUARD + nbytes + GUARD bytes, the whole block filled with the poison byte first (and, for
the ``zeros`` forms, the body zeroed after that): a kernel that reads an element it was meant to
write first sees the poison, and one that stores outside its buffer damages a guard, which
``check()`` reports.  The fills are enqueued on the current stream when the tensor is made, so they
are ordered before the launch that follows; every block stays alive until the manager is dropped,
so nothing returns to the caching allocator inside a case.

Allocations on other devices go to the real function untouched.  Forms that cannot be poisoned
(``out=``, a layout other than strided) raise instead of passing through unpoisoned, and so does
any allocation made while the current stream is being captured into a graph.

0xFF reads as NaN in every float type and as -1 / all-ones in integers; 0x5A as 1.5e16 (fp32),
1.8e127 (fp64), 203.25 (fp16) and 1515870810 (int32).  A correct kernel reads neither.
"""
import torch

GUARD = 512           # bytes before and after every poisoned tensor; keeps data_ptr() 512-byte aligned
POISONS = (0xFF, 0x5A)

_MODULE_NAMES = ("empty", "zeros", "empty_like", "zeros_like")
_METHOD_NAMES = ("new_empty", "new_zeros")


class Poison:
    """Context manager; see the module docstring.  ``device_type="cpu"`` watches CPU allocations (the
    helper's own tests)."""

    def __init__(self, byte, device_type="cuda"):
        if not 0 <= int(byte) <= 255:
            raise ValueError(f"poison byte {byte!r} out of range")
        self.byte = int(byte)
        self.device_type = device_type
        self.blocks = []      # (sequence number, whole uint8 block, nbytes, shape, dtype), kept alive
        self._saved = None

    # -- installation ---------------------------------------------------------------------------

    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("Poison is not re-entrant")
        saved = {("m", n): getattr(torch, n) for n in _MODULE_NAMES}
        # the Tensor methods live on the C base class: remember whether torch.Tensor itself had one
        saved.update({("t", n): torch.Tensor.__dict__.get(n) for n in _METHOD_NAMES})
        self._saved = saved
        self._real = {n: getattr(torch, n) for n in _MODULE_NAMES}
        self._real.update({n: getattr(torch.Tensor, n) for n in _METHOD_NAMES})
        try:
            for n in _MODULE_NAMES:
                setattr(torch, n, self._wrap(n, zero=n.startswith("zeros"), like=n.endswith("_like")))
            for n in _METHOD_NAMES:
                setattr(torch.Tensor, n, self._wrap(n, zero=n.endswith("zeros"), like=True))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        return False

    def _restore(self):
        saved, self._saved = self._saved, None
        for (kind, n), fn in saved.items():
            if kind == "m":
                setattr(torch, n, fn)
            elif fn is None:
                if n in torch.Tensor.__dict__:
                    delattr(torch.Tensor, n)
            else:
                setattr(torch.Tensor, n, fn)

    # -- the replacement ------------------------------------------------------------------------

    def _wrap(self, name, zero, like):
        real = self._real[name]

        def alloc(*args, **kwargs):
            dev = kwargs.get("device")
            if dev is None:
                dev = args[0].device if like else torch.get_default_device()
            if torch.device(dev).type != self.device_type:
                return real(*args, **kwargs)
            if kwargs.get("out") is not None:
                raise NotImplementedError(f"memcheck: torch.{name}(out=...) cannot be poisoned")
            if kwargs.get("layout", torch.strided) is not torch.strided:
                raise NotImplementedError(f"memcheck: torch.{name} with layout {kwargs['layout']} cannot be poisoned")
            if self.device_type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"memcheck: torch.{name} under a graph capture; the hook must not be active there")
            # shape, dtype and strides as the real function would choose them, without an allocation
            meta = real(*args, **dict(kwargs, device="meta", pin_memory=False))
            return self._poisoned(meta, torch.device(dev), zero, bool(kwargs.get("requires_grad", False)))

        alloc.__name__ = name
        return alloc

    def _poisoned(self, meta, device, zero, requires_grad):
        item = meta.element_size()
        span = 0
        if meta.numel():
            span = (1 + sum((n - 1) * s for n, s in zip(meta.shape, meta.stride()))) * item
        big = self._real["empty"](GUARD + span + GUARD, dtype=torch.uint8, device=device)
        big.fill_(self.byte)
        body = big[GUARD:GUARD + span]
        if zero:
            body.zero_()
        out = body.view(meta.dtype)
        out = out.view(meta.shape) if meta.is_contiguous() else out.as_strided(meta.shape, meta.stride())
        self.blocks.append((len(self.blocks), big, span, tuple(meta.shape), meta.dtype))
        if requires_grad:
            out.requires_grad_(True)
        return out

    # -- the check ------------------------------------------------------------------------------

    def check(self):
        """Synchronise, then -> [(sequence number, shape, dtype, byte offset)] of the allocations whose
        front or rear guard no longer holds the poison byte; the offset is that of the first damaged byte,
        relative to the tensor's first byte (negative: in front of it; >= its size: behind it)."""
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        damaged = []
        by_device = {}
        for blk in self.blocks:
            by_device.setdefault(blk[1].device, []).append(blk)
        for blocks in by_device.values():
            guards = torch.stack([torch.cat([big[:GUARD], big[GUARD + span:]]) for _, big, span, _, _ in blocks])
            bad = (guards != self.byte)
            rows = bad.any(dim=1).nonzero().flatten().tolist()
            for r in rows:
                seq, _, span, shape, dtype = blocks[r]
                first = int(bad[r].nonzero()[0])
                damaged.append((seq, shape, dtype, first - GUARD if first < GUARD else span + first - GUARD))
        return sorted(damaged)


def bits(t):
    """A tensor's bytes as an integer tensor on the CPU (None stays None): comparisons through it
    count NaN payloads and the sign of zero."""
    if t is None:
        return None
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8)
