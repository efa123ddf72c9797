"""A poisoning allocator shim and a call recorder for tests/test_poison_gpu.py and tests/test_poison_host.py.

Every buffer the engine writes into comes from Python as `torch.empty` (outputs, argmax arrays, plan blobs, flags, every
`*_ws_bytes` workspace).  `poisoned(word)` replaces `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty` while
it is active: a device allocation becomes the middle of a flat uint8 buffer

    [ 512 bytes guard | nbytes, rounded up to 4 | 512 bytes guard ]

filled throughout with the fill word (32-bit words; for 2-byte dtypes the 16-bit form), and the caller gets the
`[512 : 512 + nbytes]` slice viewed as the dtype and shape it asked for.  The 512-byte front guard keeps the data pointer
at the alignment torch's caching allocator gives, so the host-side kernel-form choices (`data_ptr() % 16`, strides) are
those of production.  `check_guards()` holds both guards of every buffer to the fill; a run under one fill is compared bit
for bit with the same run under another: any difference is a read of memory the launch did not write.

The fill words, always run in this order (FILLS): 0 (the baseline, through the shim too: same geometry), 1 (an index or
a counter read uninitialised becomes 1, in range for every case: the result comes out wrong, not as a wild address), and
SENTINEL of tests/_layout.py (a quiet NaN; as an integer a huge value) only after the integer-1 run matched the baseline.

Passed through untouched: `out=`, pinned memory, non-strided layouts, complex and quantised dtypes, symbolic sizes, CPU
tensors unless `cpu=True`, other device types (meta), and anything allocated while the current stream is capturing."""
import contextlib
import threading

import torch

from _bigview import SENTINEL16
from _layout import SENTINEL

GUARD = 512
FILLS = (0x00000000, 0x00000001, SENTINEL)

_ITEMSIZE = {torch.float32: 4, torch.float64: 8, torch.float16: 2, torch.bfloat16: 2, torch.int8: 1, torch.uint8: 1,
             torch.int16: 2, torch.int32: 4, torch.int64: 8, torch.bool: 1}       # the dtypes that are poisoned


def word16(word):
    """the 16-bit form of a fill word: the sentinel NaN as bf16 bits, else the low half"""
    return SENTINEL16 if word == SENTINEL else word & 0xFFFF


def word32_for(word, itemsize):
    """the 32-bit pattern a buffer of `itemsize`-byte elements is filled with"""
    if itemsize == 2:
        return (word16(word) << 16) | word16(word)
    return word & 0xFFFFFFFF


def signed(value, itemsize):
    """an unsigned bit pattern of `itemsize` bytes as the signed integer torch's int8 .. int64 hold (uint8 stays as it is)"""
    bits = 8 * itemsize
    return value - (1 << bits) if (itemsize > 1 and value >= 1 << (bits - 1)) else value


def element_pattern(word, dtype):
    """the integer every element of a freshly poisoned tensor of `dtype` holds, as an unsigned value of its width"""
    size = _ITEMSIZE[dtype]
    w = word32_for(word, size)
    if size == 1:
        return w & 0xFF            # (little endian: byte 0 of the word; every fill used here repeats or is checked whole)
    if size == 2:
        return w & 0xFFFF
    if size == 4:
        return w
    return (w << 32) | w


_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def raw_bits(t):
    """t's elements as integers of the same width (uint8 / int16 / int32 / int64), contiguous"""
    t = t.detach().contiguous()
    return t.view(_INT_OF_SIZE[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw_bits(a), raw_bits(b))


def _round4(n):
    return (n + 3) // 4 * 4


class Poison:
    """the state of one `poisoned` context: the recorded buffers, `bytes_seen`, `check_guards()`"""

    def __init__(self, word, cpu=False):
        self.word, self.cpu = int(word), bool(cpu)
        self.buffers = []              # (flat uint8 buffer, nbytes, 32-bit fill): strong references
        self.bytes_seen = 0
        self.allocations = 0
        self.passed_through = 0
        self._lock = threading.Lock()  # (backward runs on autograd's device thread)
        self._real = None

    # ---- allocation --------------------------------------------------------------------------------------------
    def _wanted(self, device, dtype, sizes):
        if dtype not in _ITEMSIZE or not all(type(s) is int for s in sizes):
            return False
        if device.type == "cpu":
            return self.cpu
        if device.type != "cuda":
            return False
        return not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())

    def alloc(self, sizes, dtype, device, requires_grad=False):
        real_empty = self._real[0]
        itemsize = _ITEMSIZE[dtype]
        n = 1
        for s in sizes:
            n *= s
        nbytes = n * itemsize
        total = GUARD + _round4(nbytes) + GUARD
        flat = real_empty(total, dtype=torch.uint8, device=device)
        w32 = word32_for(self.word, itemsize)
        flat.view(torch.int32).fill_(signed(w32, 4))
        # the front guard keeps the alignment the allocator gave: the kernels' form choices are those of production
        assert flat.data_ptr() % (GUARD if flat.is_cuda else 16) == 0, "the allocator's block is less aligned than expected"
        # a tensor of its own over the buffer's storage (no view relation for autograd to track), as torch.empty returns
        strides, acc = [], 1
        for s in reversed(sizes):
            strides.append(acc)
            acc *= max(s, 1)
        t = real_empty(0, dtype=dtype, device=flat.device).set_(flat.untyped_storage(), GUARD // itemsize, tuple(sizes),
                                                                tuple(reversed(strides)))
        assert t.is_contiguous() and t.storage_offset() * itemsize == GUARD and not t._is_view()
        assert nbytes == 0 or (t.data_ptr() == flat.data_ptr() + GUARD and t.data_ptr() % 16 == 0)
        with self._lock:
            self.buffers.append((flat, nbytes, w32))
            self.bytes_seen += nbytes
            self.allocations += 1
        return t.requires_grad_(True) if requires_grad else t

    def fill_only(self, t):
        """a tensor torch laid out itself (empty_like of a non-contiguous tensor): filled, no guards"""
        es = t.element_size()
        n = t.untyped_storage().nbytes() // es - t.storage_offset()
        flat = torch.as_strided(t.detach(), (n,), (1,))
        flat.view(_INT_OF_SIZE[es]).fill_(signed(element_pattern(self.word, t.dtype), es))
        with self._lock:
            self.bytes_seen += t.numel() * es
            self.allocations += 1
        return t

    # ---- the three replacements ----------------------------------------------------------------------------------
    def _empty(self, *size, **kw):
        real_empty = self._real[0]
        sizes = tuple(size[0]) if (len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size))) else size
        if "size" in kw and not size:
            sizes = tuple(kw["size"])
        fmt = kw.get("memory_format")
        plain = (kw.get("out") is None and not kw.get("pin_memory") and kw.get("names") is None
                 and kw.get("layout", torch.strided) in (None, torch.strided)
                 and fmt in (None, torch.contiguous_format))
        if plain:
            dtype = kw.get("dtype") or torch.get_default_dtype()
            device = torch.device(kw["device"]) if kw.get("device") is not None else torch.get_default_device()
            if self._wanted(device, dtype, sizes):
                return self.alloc(sizes, dtype, device, bool(kw.get("requires_grad", False)))
        self.passed_through += 1
        return real_empty(*size, **kw)

    def _empty_like(self, input, **kw):
        real_like = self._real[1]
        fmt = kw.get("memory_format", torch.preserve_format)
        dtype = kw.get("dtype") or input.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else input.device
        ok = (kw.get("layout") in (None, torch.strided) and input.layout == torch.strided and not kw.get("pin_memory")
              and self._wanted(device, dtype, tuple(input.shape)))
        if ok and (fmt == torch.contiguous_format or (fmt == torch.preserve_format and input.is_contiguous())):
            return self.alloc(tuple(input.shape), dtype, device, bool(kw.get("requires_grad", False)))
        out = real_like(input, **kw)
        if ok and fmt == torch.preserve_format:
            return self.fill_only(out)
        self.passed_through += 1
        return out

    def _new_empty(self, tensor, *size, **kw):
        real_new = self._real[2]
        sizes = tuple(size[0]) if (len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size))) else size
        if "size" in kw and not size:
            sizes = tuple(kw["size"])
        dtype = kw.get("dtype") or tensor.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else tensor.device
        if (kw.get("layout") in (None, torch.strided) and tensor.layout == torch.strided and not kw.get("pin_memory")
                and type(tensor) is torch.Tensor and self._wanted(device, dtype, sizes)):
            return self.alloc(sizes, dtype, device, bool(kw.get("requires_grad", False)))
        self.passed_through += 1
        return real_new(tensor, *size, **kw)

    # ---- checks ------------------------------------------------------------------------------------------------
    def check_guards(self):
        """both guards (and the round-up slack) of every recorded buffer still hold the fill word"""
        bad = []
        for i, (flat, nbytes, w32) in enumerate(self.buffers):
            pat = torch.tensor([(w32 >> (8 * k)) & 0xFF for k in range(4)], dtype=torch.uint8, device=flat.device)
            front = flat[:GUARD].view(-1, 4)
            tail0 = GUARD + _round4(nbytes)
            tail = flat[tail0:].view(-1, 4)
            slack = flat[GUARD + nbytes:tail0]
            n_bad = int((front != pat).sum()) + int((tail != pat).sum())
            if slack.numel():
                n_bad += int((slack != pat[4 - slack.numel():]).sum())
            if n_bad:
                before = int((front != pat).any())
                bad.append(f"allocation {i} ({nbytes} bytes): {n_bad} guard bytes overwritten "
                           f"({'before' if before else 'behind'} the tensor)")
        assert not bad, "; ".join(bad[:8])


@contextlib.contextmanager
def poisoned(word, cpu=False):
    """replace torch.empty, torch.empty_like and torch.Tensor.new_empty by the poisoning forms; restored on exit, also
    after an exception.  Yields the Poison that records the buffers."""
    p = Poison(word, cpu)
    own_new = "new_empty" in torch.Tensor.__dict__
    p._real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    real = p._real
    torch.empty = p._empty
    torch.empty_like = p._empty_like
    torch.Tensor.new_empty = lambda self, *a, **k: p._new_empty(self, *a, **k)
    try:
        yield p
    finally:
        torch.empty, torch.empty_like = real[0], real[1]
        if own_new:
            torch.Tensor.new_empty = real[2]
        else:
            del torch.Tensor.new_empty


class Recorder:
    """stands in for the loaded library (`monkeypatch.setattr(_lib, "_lib", Recorder(real))`): records the name of every
    C entry that is fetched and hands out the real function"""

    def __init__(self, real):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "seen", [])

    def __getattr__(self, name):
        fn = getattr(object.__getattribute__(self, "_real"), name)
        if name.startswith("mp_"):
            object.__getattribute__(self, "seen").append(name)
        return fn

    def names(self):
        return set(object.__getattribute__(self, "seen"))


def fill_hits(run, base, word):
    """elements of `run` that hold the fill's bit pattern where the baseline does not (0 for the baseline fill itself)"""
    bits_r, bits_b = raw_bits(run), raw_bits(base)
    pat = signed(element_pattern(word, run.dtype), bits_r.element_size())
    return int(((bits_r == pat) & (bits_b != pat)).sum())
