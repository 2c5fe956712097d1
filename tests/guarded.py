"""Device outputs inside larger sentinel-filled buffers (GPU tests): a kernel that writes before or after its
declared extent changes a guard element, and one that leaves part of its extent unwritten leaves the sentinel
where the reference has a value."""
import numpy as np
import torch

GUARD = 64
SENTINELS = {torch.int32: -7777, torch.int64: -7777, torch.float32: -7777.0, torch.uint8: 0xA5}


class Guarded:
    """A contiguous `shape` view of `dtype` (`.view`, `.ptr` address) with GUARD sentinel elements on either side.
    GUARD elements of every dtype used are a multiple of 16 bytes, so the view keeps the allocation's alignment."""

    def __init__(self, dev, shape, dtype=torch.int32):
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape))
        self.sentinel = SENTINELS[dtype]
        self.full = torch.full((self.n + 2 * GUARD,), self.sentinel, dtype=dtype, device=dev)
        self.view = self.full[GUARD:GUARD + self.n].view(self.shape)
        # not view.data_ptr(): an empty view (a rejected N = 0 call) would report a null address
        self.ptr = self.full.data_ptr() + GUARD * self.full.element_size()

    def get(self) -> np.ndarray:
        """The view's contents (host), after checking that both guards still hold the sentinel."""
        h = self.full.cpu().numpy()
        assert (h[:GUARD] == self.sentinel).all(), "write before the declared extent"
        assert (h[GUARD + self.n:] == self.sentinel).all(), "write after the declared extent"
        return h[GUARD:GUARD + self.n].reshape(self.shape)

    def untouched(self) -> bool:
        return bool((self.full == self.sentinel).all())
