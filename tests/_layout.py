"""Operand layouts for tests/test_layouts_gpu.py: column slices of wider device buffers.

An operand of width d lives at columns off .. off + d of an [n, ld] buffer, so its rows are ld elements apart and its
first element sits 4 * off bytes past a 16-byte boundary.  Output buffers are filled with a sentinel bit pattern (a NaN
with a payload: no arithmetic produces it) and `assert_untouched` checks that every element outside the slice still
holds exactly those bits; inputs are compared bit for bit with a clone taken before the call."""
import torch

SENTINEL = 0x7FC5A5A5           # a quiet NaN with a payload; as int32 it is far outside any entry index

# (name, ld - d, off): the set every operator is run on
LAYOUTS = [
    ("contig", 0, 0),           # the baseline
    ("ld+4", 4, 0),             # strided, rows still 16-byte aligned
    ("ld+8,off4", 8, 4),
    ("ld+4,off2", 4, 2),        # 8-byte aligned base
    ("ld+4,off1", 4, 1),        # 4-byte aligned base
    ("ld+5,off3", 5, 3),
    ("ld+3", 3, 0),             # aligned base, odd leading dimension: rows alternate alignment
    ("ld+1", 1, 0),
]
CONTIG = LAYOUTS[0]
OFF1 = LAYOUTS[4]               # the misaligned layout of the mixed cases (one operand off, the others aligned)
ALIGNED = {"contig", "ld+4", "ld+8,off4"}     # rows on 16-byte boundaries: the vector form of every kernel


def _check(buf, v, d, ld, off):
    """the case is the one it claims to be, whatever torch's allocator does"""
    assert buf.data_ptr() % 16 == 0
    assert v.stride(0) == ld and v.stride(1) == 1 and v.size(1) == d
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    return buf, v


def view(n, d, ld, off, seed, dev, dtype=torch.float32):
    """(buf, v): an [n, ld] device buffer of random values and its column slice v = buf[:, off:off + d]"""
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        buf = torch.randn(n, ld, generator=g).to(dtype).to(dev)
    else:
        buf = torch.randint(-3, 1 << 20, (n, ld), generator=g).to(dtype).to(dev)
    return _check(buf, buf[:, off:off + d], d, ld, off)


def view_of(t, layout, dev, seed=0):
    """(buf, v) with v holding the values of the 2-D tensor t in the given layout (the rest of buf: random values)"""
    _, extra, off = layout
    n, d = t.shape
    buf, v = view(n, d + extra, d + extra, 0, seed + 1000, dev, t.dtype)
    v = buf[:, off:off + d]
    v.copy_(t)
    return _check(buf, v, d, d + extra, off)


def out_view(n, d, layout, dev, dtype=torch.float32):
    """(buf, v): a sentinel-filled [n, d + extra] output buffer and the slice a kernel is to write"""
    _, extra, off = layout
    assert dtype in (torch.float32, torch.int32)
    buf = torch.full((n, d + extra), SENTINEL, dtype=torch.int32, device=dev).view(dtype)
    return _check(buf, buf[:, off:off + d], d, d + extra, off)


def assert_untouched(buf, off, d, what=""):
    """every element of buf outside columns off .. off + d still holds the sentinel's bits"""
    bits = buf.view(torch.int32)
    keep = torch.ones(buf.size(1), dtype=torch.bool, device=buf.device)
    keep[off:off + d] = False
    bad = bits[:, keep] != SENTINEL
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beside the output slice were overwritten"


def assert_all_sentinel(buf, what=""):
    assert bool((buf.view(torch.int32) == SENTINEL).all()), f"{what}: a refused call wrote to its output"


def assert_written(v, what=""):
    """no element of the slice was left out"""
    assert not bool((v.view(torch.int32) == SENTINEL).any()), f"{what}: part of the output slice was not written"


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Unchanged:
    """`with Unchanged(buf_x, buf_s): call(...)` — the input buffers (slice and surroundings) keep their bits"""
    def __init__(self, *bufs):
        self.bufs = [b for b in bufs if b is not None]

    def __enter__(self):
        self.before = [b.clone() for b in self.bufs]
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            torch.cuda.synchronize()
            for i, (b, c) in enumerate(zip(self.bufs, self.before)):
                assert same_bits(b, c), f"input {i} was modified"
        return False
