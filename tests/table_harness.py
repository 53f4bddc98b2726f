"""What the GPU tests of the families outside Filter share (test_hist_gpu.py, test_clahe_gpu.py, test_arith_gpu.py,
test_box_gpu.py, test_dist_gpu.py): the stream, an input on the device at a byte offset, and an output, table or work
buffer on the device inside guard elements that are checked when it is read back."""
import numpy as np


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def upload(torch, host, offset=0):
    """host at `offset` bytes into a zeroed device buffer with 64 spare bytes; (tensor, address of the data)."""
    host = np.ascontiguousarray(host)
    d = torch.zeros(host.size * host.itemsize + 64, dtype=torch.uint8, device="cuda")
    d[offset:offset + host.size * host.itemsize] = torch.from_numpy(host.reshape(-1).view(np.uint8)).cuda()
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + offset


class Guarded:
    """n elements of dtype (np.uint8 | np.uint32) on the device with `front` guard elements before them and `back` behind,
    the whole buffer filled with `fill`.  ptr: the address of the n elements (the buffer's own is 16-byte aligned);
    payload(): the n elements from the device, after asserting that every guard still holds `fill`: "wrote outside " + what."""

    def __init__(self, torch, n, what, dtype=np.uint8, fill=0x5A, front=0, back=64):
        self.n, self.what, self.dtype, self.fill, self.front = n, what, np.dtype(dtype), fill, front
        kind, signed = {1: (torch.uint8, fill), 4: (torch.int32, fill - (1 << 32) if fill >= 1 << 31 else fill)}[self.dtype.itemsize]
        self.tensor = torch.full((front + n + back,), signed, dtype=kind, device="cuda")
        assert self.tensor.data_ptr() % 16 == 0
        self.ptr = self.tensor.data_ptr() + front * self.dtype.itemsize

    def payload(self):
        o = self.tensor.cpu().numpy().view(self.dtype)
        at = self.front
        assert (o[:at] == self.fill).all() and (o[at + self.n:] == self.fill).all(), "wrote outside " + self.what
        return o[at:at + self.n]
