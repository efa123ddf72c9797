"""Operands for tests/test_bigoffset_gpu.py: column slices of device buffers so wide that a row's offset passes 2^32 bytes
and 2^31 elements.

A buffer is [n, ld] with n = 70 000 and ld = 32 768 (or 32 771): in fp32 rows >= 32 768 lie past 2^32 bytes and rows
>= 65 536 past 2^31 elements; in bf16 both thresholds fall at row 65 536.  Buffers are allocated on the device, filled with
the sentinel NaN of tests/_layout.py in one fill (inputs too: a stray read shows as a NaN in the result, a stray write as a
changed sentinel), and only the slice is given values.  Nothing of size [n, ld] is ever built on the host, and the checks
on a whole buffer run in row chunks."""
import pytest
import torch

from _layout import SENTINEL

N_WIDE = 70_000
ROW_BYTES32 = 32_768            # first fp32 row past 2^32 bytes
ROW_ELEMS31 = 65_536            # first row past 2^31 elements (and past 2^32 bytes in bf16)
SENTINEL16 = SENTINEL >> 16     # 0x7FC5: the same quiet NaN as bf16 bits

# (name, ld, off): 16-byte aligned rows (the vector / tile / MFMA forms) and the scalar / row-kernel fallbacks
WIDE = [("aligned", 32_768, 0), ("misaligned", 32_771, 1)]
IDS = [w[0] for w in WIDE]


def need(nbytes, what=""):
    """skip (with the byte counts) when the device has less free memory than the case allocates"""
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what}: needs {nbytes} bytes of device memory, {free} of {total} free")


def _bits(buf):
    return buf.view(torch.int16 if buf.element_size() == 2 else torch.int32)


def _sentinel(buf):
    return SENTINEL16 if buf.element_size() == 2 else SENTINEL


def wide_empty(n, d, lay, dev, dtype=torch.float32):
    """(buf, v): a sentinel-filled [n, ld] device buffer and its slice v = buf[:, off:off + d]"""
    _, ld, off = lay
    if dtype == torch.bfloat16:
        buf = torch.empty((n, ld), dtype=torch.int16, device=dev).fill_(SENTINEL16).view(dtype)
    else:
        assert dtype in (torch.float32, torch.int32)
        buf = torch.empty((n, ld), dtype=torch.int32, device=dev).fill_(SENTINEL).view(dtype)
    v = buf[:, off:off + d]
    assert buf.data_ptr() % 16 == 0 and v.stride(0) == ld and v.stride(1) == 1 and v.shape == (n, d)
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    if n == N_WIDE:             # the case is the one it claims to be
        assert ROW_ELEMS31 * ld >= 1 << 31                                   # elements, either dtype
        assert (ROW_ELEMS31 * ld * 2 if dtype == torch.bfloat16 else ROW_BYTES32 * ld * 4) >= 1 << 32        # bytes
    return buf, v


def wide_of(t, lay, dev):
    """(buf, v) with v holding the values of the 2-D tensor t (host or device); the rest of buf is the sentinel"""
    buf, v = wide_empty(t.size(0), t.size(1), lay, dev, t.dtype)
    v.copy_(t)
    return buf, v


def assert_beside(buf, lay, d, what="", rows=2048):
    """every element of buf outside the slice still holds the sentinel's bits; row chunks of `rows` keep the check's own
    memory at rows x ld bytes (64 MiB)"""
    _, ld, off = lay
    bits, s = _bits(buf), _sentinel(buf)
    bad = torch.zeros((), dtype=torch.int64, device=buf.device)
    for r0 in range(0, buf.size(0), rows):
        c = bits[r0:r0 + rows]
        if off:
            bad += (c[:, :off] != s).sum()
        bad += (c[:, off + d:] != s).sum()
    assert int(bad) == 0, f"{what}: {int(bad)} elements beside the slice were overwritten"


def assert_written(v, what=""):
    assert not bool((_bits_of_slice(v) == _sentinel(v)).any()), f"{what}: part of the output slice was not written"


def _bits_of_slice(v):
    return v.contiguous().view(torch.int16 if v.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits_of_slice(a), _bits_of_slice(b))


class Kept:
    """`with Kept((buf, v, lay), ...): call(...)`: every input buffer keeps its bits — the slice against a copy taken
    before the call, the rest against the sentinel"""
    def __init__(self, *ops):
        self.ops = [o for o in ops if o is not None and o[0] is not None]

    def __enter__(self):
        self.before = [v.clone() for _, v, _ in self.ops]
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            torch.cuda.synchronize()
            for i, ((buf, v, lay), c) in enumerate(zip(self.ops, self.before)):
                assert same_bits(v, c), f"input {i} was modified"
                assert_beside(buf, lay, v.size(1), f"input {i}")
        return False


def sample_rows(n, extra=(), k=48, seed=0):
    """sorted unique rows to check: both sides of both thresholds, the first and last row, `extra`, and k random ones"""
    fixed = [0, 1, n - 1, n - 2]
    for t in (ROW_BYTES32, ROW_ELEMS31):
        if t < n:
            fixed += [t - 2, t - 1, t, t + 1]
    rnd = torch.randint(0, n, (k,), generator=torch.Generator().manual_seed(seed))
    rows = torch.unique(torch.cat([torch.tensor(fixed + list(extra), dtype=torch.int64), rnd]))
    assert bool((rows >= 0).all()) and bool((rows < n).all())
    return rows
