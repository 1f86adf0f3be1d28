"""Guarded device buffers for tests that call the C entries directly (tests/test_hip_latent_counts.py, tests/test_hip_style_demod.py).

An operand lies at the head of a larger NaN-filled allocation: a read with a wrong stride or offset pulls NaN into the result instead of
a neighbour's plausible numbers, and stays inside the allocation.  An output is NaN before the call and is followed by a NaN guard that
must still be NaN after it: a write with a wrong stride either leaves NaN inside or lands in the guard."""
import numpy as np
import torch

NAN = float("nan")


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


INT_FILL = {torch.int32: -1515870811}        # the "nothing was written here" pattern of the integer variant (0xA5 bytes)


class Guarded:
    """A float32 device tensor `t` at the head of a NaN-filled buffer.  span = 16: room for a [rows][T] table read or written with row
    stride 16 (the padded width of the kernels' tables); span = 1: 64 floats behind the end.
    dtype: float64 likewise; an int32 buffer is filled with INT_FILL's pattern instead of NaN (a value no test writes on purpose)."""

    def __init__(self, shape, data=None, span=1, offset=0, dtype=torch.float32):
        numel = int(np.prod(shape))
        self.fill = NAN if dtype.is_floating_point else INT_FILL[dtype]
        self.buf = torch.full((offset + numel * span + 64,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[offset:offset + numel].view(*shape)
        self.end = offset + numel
        if data is not None:
            self.t.copy_(torch.as_tensor(data).detach().to(dtype))

    def ptr(self):
        return self.t.data_ptr()

    def _blank(self, x):
        return torch.isnan(x) if x.dtype.is_floating_point else x == self.fill

    def guard_intact(self):
        return bool(self._blank(self.buf[self.end:]).all())

    def written(self):
        return not bool(self._blank(self.t).any())

    def numpy(self):
        return self.t.detach().cpu().numpy()


def g_in(t64, span=1):
    return Guarded(tuple(t64.shape), t64, span)


def g_out(*shape, span=1):
    return Guarded(shape, None, span)


def device_table(jobs, kind):
    """A device array of job records (ctypes structures of type `kind`), uploaded the way engine.py and grad.py upload theirs."""
    from morphganformer_amd import _lib
    return _lib.device_table((kind * len(jobs))(*jobs), "cuda")
