"""tests/memcheck.py on CPU tensors (the device filter pointed at "cpu"): the poison patterns per
dtype, the guards, what check() reports and that the hook leaves torch as it found it."""
import struct

import pytest
import torch

import memcheck
from memcheck import GUARD, Poison

# what the two poison bytes read as, per dtype (None: NaN)
PATTERNS = {
    0xFF: {torch.float16: None, torch.float32: None, torch.float64: None, torch.int32: -1, torch.int64: -1,
           torch.uint8: 255},
    0x5A: {torch.float16: 203.25, torch.float32: struct.unpack("<f", b"\x5a" * 4)[0],      # 1.5e16
           torch.float64: struct.unpack("<d", b"\x5a" * 8)[0],                               # 1.8e127
           torch.int32: 1515870810, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A},
}
assert 1.5e16 < PATTERNS[0x5A][torch.float32] < 1.6e16 and 1.7e127 < PATTERNS[0x5A][torch.float64] < 1.8e127


@pytest.mark.parametrize("byte", memcheck.POISONS)
@pytest.mark.parametrize("dtype", sorted(PATTERNS[0xFF], key=str))
def test_fill_per_dtype(byte, dtype):
    with Poison(byte, "cpu") as mc:
        t = torch.empty(3, 5, dtype=dtype, device="cpu")
        u = torch.empty((7,), dtype=dtype)            # default device, size as a tuple
    assert t.shape == (3, 5) and t.dtype == dtype and t.is_contiguous() and u.shape == (7,)
    want = PATTERNS[byte][dtype]
    for x in (t, u):
        if want is None:
            assert bool(torch.isnan(x).all())
        elif dtype.is_floating_point:
            assert bool((x == torch.tensor(want, dtype=torch.float64).to(dtype)).all()), x.flatten()[0]
        else:
            assert bool((x == want).all()), x.flatten()[0]
    assert bool((memcheck.bits(t) == byte).all())
    assert mc.check() == [] and len(mc.blocks) == 2
    seq, big, span, shape, dt = mc.blocks[0]
    assert (seq, span, shape, dt) == (0, 15 * t.element_size(), (3, 5), dtype)
    assert big.numel() == 2 * GUARD + span and t.data_ptr() == big.data_ptr() + GUARD


@pytest.mark.parametrize("byte", memcheck.POISONS)
def test_zeros_stay_zero_inside_the_guards(byte):
    with Poison(byte, "cpu") as mc:
        z = torch.zeros(4, 9, dtype=torch.float64)
        zl = torch.zeros_like(z)
        nz = z.new_zeros(5, dtype=torch.int32)
        el = torch.empty_like(z[:, ::2].t())           # dense but permuted: strides kept
        ne = z.new_empty((2, 3))
    for t in (z, zl, nz):
        assert bool((memcheck.bits(t) == 0).all())
    assert bool((memcheck.bits(ne) == byte).all()) and ne.dtype == torch.float64
    assert el.shape == (5, 4) and bool((memcheck.bits(el) == byte).all())
    for _, big, span, _, _ in mc.blocks:
        assert bool((big[:GUARD] == byte).all()) and bool((big[GUARD + span:] == byte).all())
    assert mc.check() == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.uint8])
def test_store_past_the_end_is_caught(dtype):
    with Poison(0x5A, "cpu") as mc:
        torch.empty(8, dtype=torch.float32)
        t = torch.empty(6, 3, dtype=dtype)
        torch.zeros(2)
    torch.as_strided(t, (1,), (1,), t.storage_offset() + t.numel()).zero_()
    assert mc.check() == [(1, (6, 3), dtype, 18 * t.element_size())]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.uint8])
def test_store_before_the_start_is_caught(dtype):
    with Poison(0xFF, "cpu") as mc:
        t = torch.zeros(6, 3, dtype=dtype)
    torch.as_strided(t, (1,), (1,), t.storage_offset() - 1).zero_()
    assert mc.check() == [(0, (6, 3), dtype, -t.element_size())]


def test_stores_inside_report_nothing():
    with Poison(0xFF, "cpu") as mc:
        t = torch.empty(1000, dtype=torch.float32)
        t.copy_(torch.arange(1000.0))
        t[-1] = 0.0
        t[0] = 0.0
    assert mc.check() == []


def test_zero_size():
    with Poison(0x5A, "cpu") as mc:
        a = torch.empty(0, dtype=torch.float32)
        b = torch.zeros(4, 0, 3, dtype=torch.int64)
        c = torch.empty_like(b)
    assert a.shape == (0,) and b.shape == (4, 0, 3) and c.shape == (4, 0, 3) and c.dtype == torch.int64
    assert [blk[2] for blk in mc.blocks] == [0, 0, 0] and mc.check() == []
    mc.blocks[1][1][GUARD] = 0                        # the first byte behind an empty tensor
    assert mc.check() == [(1, (4, 0, 3), torch.int64, 0)]


def test_other_devices_and_unpoisonable_forms():
    with Poison(0xFF, "cuda") as mc:                  # watching the GPU: CPU allocations pass through
        t = torch.zeros(5)
        assert bool((t == 0).all()) and t._base is None
    assert mc.blocks == []
    with Poison(0xFF, "cpu"):
        with pytest.raises(NotImplementedError):
            torch.empty(3, out=torch.empty(3, device="meta"), device="cpu")
        with pytest.raises(NotImplementedError):
            torch.zeros(3, 3, layout=torch.sparse_coo)
        m = torch.empty(3, device="meta")             # another device
        assert m.device.type == "meta"


def test_originals_restored():
    names = ("empty", "zeros", "empty_like", "zeros_like")
    before = [getattr(torch, n) for n in names]
    methods = [torch.Tensor.new_empty, torch.Tensor.new_zeros]
    had = ["new_empty" in torch.Tensor.__dict__, "new_zeros" in torch.Tensor.__dict__]
    with Poison(0xFF, "cpu"):
        assert all(getattr(torch, n) is not f for n, f in zip(names, before))
        assert torch.Tensor.new_empty is not methods[0]
    assert all(getattr(torch, n) is f for n, f in zip(names, before))
    with pytest.raises(KeyError):
        with Poison(0x5A, "cpu"):
            raise KeyError("inside the block")
    assert all(getattr(torch, n) is f for n, f in zip(names, before))
    assert [torch.Tensor.new_empty, torch.Tensor.new_zeros] == methods
    assert ["new_empty" in torch.Tensor.__dict__, "new_zeros" in torch.Tensor.__dict__] == had
    assert torch.empty(3).untyped_storage().nbytes() == 12   # the real allocator again: no guards
