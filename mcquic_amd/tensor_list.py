"""The host side of csrc/tensor_list.h: the device tables the whole-model kernels walk, named after the structs there.  `ChunkTable` is
McqChunkTable (sizes and chunks: all the gradient gather needs), `TensorList` is McqTensorList (the pointer rows on top), as the
optimizers and the weight average of `optim` pass them."""
from __future__ import annotations

import torch

from . import _lib


def chunk_tables(sizes):
    """The host side of the chunk tables the whole-model kernels walk (csrc/tensor_list.h), for tensors of `sizes` elements:
    (blk_tensor, blk_first, tensor_first_blk) -- one (tensor, first element) entry per chunk of mcq_adam_chunk() elements, in tensor
    order, and [len(sizes) + 1] chunk offsets: tensor i owns the chunks [tensor_first_blk[i], tensor_first_blk[i + 1]); a tensor
    without elements owns none."""
    chunk = _lib.load().mcq_adam_chunk()
    blk_tensor, blk_first, tensor_first_blk = [], [], [0]
    for i, n in enumerate(sizes):
        for first in range(0, n, chunk):
            blk_tensor.append(i)
            blk_first.append(first)
        tensor_first_blk.append(len(blk_tensor))
    return blk_tensor, blk_first, tensor_first_blk


def flat_layout(sizes):
    """(offsets, total) of tensors of `sizes` elements laid out in ONE flat float32 buffer, every slice 16-byte aligned."""
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += (n + 3) // 4 * 4
    return offsets, at


class ChunkTable:
    """`numel` [ntensors] int64, `blk_tensor` [nblocks] int32 and `blk_first` [nblocks] int64 on `device`: they depend on the sizes only."""

    def __init__(self, sizes, device):
        self.sizes, self.ntensors = list(sizes), len(sizes)
        blk_t, blk_f, self._first_blk = chunk_tables(self.sizes)
        self.numel = torch.tensor(self.sizes, dtype=torch.int64).to(device)
        self.blk_tensor = torch.tensor(blk_t, dtype=torch.int32).to(device)
        self.blk_first = torch.tensor(blk_f, dtype=torch.int64).to(device)
        self.nblocks = len(blk_t)

    @property
    def tensor_first_blk(self) -> torch.Tensor:
        """[ntensors + 1] int32 chunk offsets, uploaded on first use (only LAMB's per-tensor norms walk them)."""
        if not torch.is_tensor(self._first_blk):
            self._first_blk = torch.tensor(self._first_blk, dtype=torch.int32).to(self.numel.device)
        return self._first_blk


class TensorList(ChunkTable):
    """The chunk table plus `rows` pointer rows (row k of tensor t at ptrs[k * ntensors + t]) in ONE int64 device buffer for the
    object's lifetime, refilled in place: a captured graph that reads it keeps a valid address and sees the current pointers.
    `moved` heads the error of a refill attempted inside a capture: who the caller is and which addresses changed."""

    def __init__(self, sizes, device, rows: int = 4, moved: str = "mcquic_amd.tensor_list: addresses changed"):
        super().__init__(sizes, device)
        self.ptrs = torch.zeros(rows * self.ntensors, dtype=torch.int64, device=device)
        self._moved, self._held = moved, ()

    def fill(self, *rows) -> None:
        """Rows 0 .. len(rows) - 1 point at these lists of tensors (None: a row of zeros); rows behind them keep what they hold, so
        the rows a caller owns are filled once and only the ones that can move are passed on every call.  Uploads only when an
        address differs from what the buffer holds."""
        zeros = (0,) * self.ntensors
        addrs = tuple(a for row in rows for a in (zeros if row is None else map(torch.Tensor.data_ptr, row)))
        if len(addrs) != len(rows) * self.ntensors or len(addrs) > self.ptrs.numel():
            raise ValueError(f"mcquic_amd.tensor_list: a row holds one tensor per size ({self.ntensors}), and the buffer {self.ptrs.numel()} pointers")
        if self._held[:len(addrs)] == addrs:
            return
        if self.ptrs.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._moved}; call `prepare()` before capturing (a host-to-device copy of the pointer table cannot be "
                               "part of a graph)")
        self.ptrs[:len(addrs)].copy_(torch.tensor(addrs, dtype=torch.int64))       # (stream-ordered behind the launches that read the old one)
        self._held = addrs + self._held[len(addrs):]

    def args(self, first_blk: bool = False) -> tuple:
        """The leading arguments of every entry point that walks the list; `first_blk`: with tensor_first_blk in front of nblocks,
        as mcq_lamb_step_f32 takes them."""
        head = (self.ptrs.data_ptr(), self.ntensors, self.numel.data_ptr(), self.blk_tensor.data_ptr(), self.blk_first.data_ptr())
        return head + ((self.tensor_first_blk.data_ptr(), self.nblocks) if first_blk else (self.nblocks,))
