"""NaN-filled device buffers with guard space, and bitwise equality: shared by the GPU tests that check what a launch
writes AND what it leaves alone."""
import torch

DEV = "cuda"
NAN = float("nan")


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    as_int = torch.int32 if a.element_size() == 4 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


class Padded:
    """`.view`: rows x cols at the top left of a NaN-filled device buffer that is `extra` columns wider and two rows
    longer; a launch may touch nothing of the buffer but the view."""

    def __init__(self, rows, cols, extra, dtype=torch.float32, fill=None):
        self.buf = torch.full((rows + 2, cols + extra), NAN, dtype=dtype, device=DEV)
        self.view = self.buf[:rows, :cols]
        if fill is not None:
            self.view.copy_(fill)

    def untouched(self) -> bool:
        rows, cols = self.view.shape
        return bool(torch.isnan(self.buf[:rows, cols:]).all() and torch.isnan(self.buf[rows:]).all())
