"""Two ways of driving the SAME C-ABI entry points with the SAME test bodies:
  EmuBackend — host-emulated build of the kernel sources (tests/emu), numpy buffers, CPU test tier;
  HipBackend — the real gfx950 library, torch CUDA tensors, `-m gpu` tier.

GUARD BANDS.  Every buffer a backend hands out is the middle of one larger block

    [ front guard | payload (exactly the requested bytes) | back guard ]

The payload starts on a 16-byte boundary (the library requires it) and the back guard starts at the first byte after it: nothing is
rounded up.  Both guards are GUARD_BYTES long and filled with a poison word; `check_guards` compares every guard of every live block
with its poison bit for bit, after EVERY library call that takes a stream (be.lib is wrapped: GuardedCalls) and before every
read-back (be.np / be.raw) — a kernel that stores outside the tensors it was given fails the test at the call that did it, with the
buffer, the side and the byte offset.  An out-of-bounds READ that reaches a result poisons it:
  POISON_NAN — a quiet NaN (the default): every comparison of the case files fails on NaN;
  POISON_BIG — 1e38 as a float, large and odd as an int32 / a fixed-point int64: for the reductions that skip NaN by design (absmax, the
               *_max forms, the plane producers' max words, maxpool); those cases run under both (`both_poisons`).
Four bits of the word differ from one allocation to the next, so poison carried from one buffer's guard into another's is seen too.
GUARD_BYTES: the widest deliberate over-read in the sources is the 16 KiB scratch slack of conv_split16.hip and the longest row of any
case is 1024 floats = 4 KiB, so 64 KiB covers a 16-row overrun at the largest shape."""
import contextlib
import ctypes
import functools
import weakref

import numpy as np

from side_inputs import SideInputs

GUARD_BYTES = 64 * 1024
POISON_NAN = 0x7fc5a5a5
POISON_BIG = 0x7e967699          # 1e38f; 2123789977 as int32 (odd); 0x7e9676997e967699 as int64
POISONS = (POISON_NAN, POISON_BIG)
POISON_VARIANTS = 16             # bits 8..11 of the word count the allocations: a kernel that carries one buffer's poison across the end of
                                 # another (out[n] = a[n] + b[n]: a NaN keeps its payload) still changes the guard it lands in

# entry points whose last argument is a pointer but not a stream: no launch, no check
_NOT_LAUNCHES = ("nemar_set_dropout_base", "nemar_tune_ptr", "nemar_kernel_timer_read")


@functools.lru_cache(maxsize=None)
def _pattern(word, phase, n=GUARD_BYTES):
    """n poison bytes as they lie in memory from an address that is `phase` bytes past a 4-byte boundary: an aligned 32-bit load anywhere
    in a guard sees the whole word"""
    b = np.frombuffer(np.uint32(word).tobytes(), dtype=np.uint8)
    p = np.tile(b, n // 4 + 2)[phase:phase + n].copy()
    p.setflags(write=False)
    return p


class _Block:
    """one guarded allocation: where its guards lie and what they must hold"""
    __slots__ = ("ref", "start", "nbytes", "shape", "dtype", "role", "poison", "__weakref__")

    def describe(self):
        return "%s buffer, shape %s %s, %d bytes" % (self.role, tuple(self.shape), self.dtype, self.nbytes)


def _launches(lib, full):
    from nemar_amd import _lib as L
    sig = L.SIGNATURES.get(full) or L.AB_SIGNATURES.get(full)
    if sig is None or full in _NOT_LAUNCHES:
        return False
    res, args = sig
    return res is ctypes.c_int and len(args) >= 2 and args[-1] is ctypes.c_void_p


class GuardedCalls:
    """The library with every launching entry point followed by a device sync and a guard check that carries the entry point's name."""

    def __init__(self, lib, be):
        self._lib, self._be = lib, be

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        full = name if name.startswith("nemar_") else "nemar_" + name
        if not callable(fn) or not _launches(self._lib, full):
            return fn
        be = self._be

        def guarded(*a):
            rc = fn(*a)
            be.sync()
            be.check_guards(full)
            return rc

        guarded.__name__ = full
        self.__dict__[name] = guarded
        return guarded


class _Guarded:
    """what the two backends share: the registry of live blocks, the poison in force, the check"""
    guard_bytes = GUARD_BYTES

    def _init_guards(self, lib):
        self.poison = POISON_NAN
        self._blocks = []
        self.checks = 0
        self.lib = SideInputs(GuardedCalls(lib, self))      # (registered side inputs -> the per-call form of the C ABI)

    @contextlib.contextmanager
    def poisoned(self, word):
        """buffers allocated inside the block carry `word` in their guards"""
        old, self.poison = self.poison, word
        try:
            yield self
        finally:
            self.poison = old

    def _register(self, ref, start, nbytes, shape, dtype, role):
        b = _Block()
        b.ref, b.start, b.nbytes, b.shape, b.dtype, b.role, b.poison = ref, start, nbytes, shape, str(dtype), role, self._next_poison()
        self._blocks.append(b)
        return b

    def _next_poison(self):
        """the poison in force, bits 8..11 replaced by a running count (still a quiet NaN / still ~1e38 and odd)"""
        self._serial = (getattr(self, "_serial", 0) + 1) % POISON_VARIANTS
        return (self.poison & ~0xf00) | (self._serial << 8)

    def poison_of(self, h):
        """the poison word in the guards of handle h's block"""
        return self._block_of(h).poison

    def live_blocks(self):
        self._blocks = [b for b in self._blocks if b.ref() is not None]
        return self._blocks

    def _fail(self, b, side, idx, got, want, what):
        off = idx - GUARD_BYTES if side == "front" else b.nbytes + idx
        self._blocks.remove(b)            # reported once: a later call is not blamed for it (a failed test's traceback keeps its buffers alive)
        raise AssertionError("guard band corrupted after %s: %s, %s guard, first bad byte at payload offset %+d (0x%02x, poison byte 0x%02x)"
                             % (what, b.describe(), side, off, got, want))

    def _locate(self, b, front, back, what):
        """front / back: the guards' bytes on the host"""
        for side, got, want in (("front", front, _pattern(b.poison, 0)), ("back", back, _pattern(b.poison, b.nbytes % 4))):
            bad = np.flatnonzero(got != want)
            if bad.size:
                self._fail(b, side, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), what)


def both_poisons(case):
    """Run a case body twice: under the NaN poison and under the large finite one (reductions that ignore NaN by design)."""
    @functools.wraps(case)
    def run(be, *a, **k):
        for word in POISONS:
            with be.poisoned(word):
                case(be, *a, **k)
    return run


class EmuBackend(_Guarded):
    name = "emu"
    stream = None

    def __init__(self, lib):
        self._init_guards(lib)

    # ---- guarded allocation ----
    def _alloc(self, shape, dtype, role):
        shape = tuple(int(s) for s in shape)
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        raw = np.empty(2 * GUARD_BYTES + nbytes + 16, dtype=np.uint8)
        start = (-(raw.ctypes.data + GUARD_BYTES)) % 16          # the payload on a 16-byte boundary
        b = self._register(weakref.ref(raw), start, nbytes, shape, dtype, role)
        raw[start:start + GUARD_BYTES] = _pattern(b.poison, 0)
        raw[start + GUARD_BYTES + nbytes:start + 2 * GUARD_BYTES + nbytes] = _pattern(b.poison, nbytes % 4)
        return raw[start + GUARD_BYTES:start + GUARD_BYTES + nbytes].view(dtype).reshape(shape)      # (.base is `raw`: alive while any view is)

    def _from(self, a, dtype, role):
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        h = self._alloc(a.shape, dtype, role)
        h[...] = a
        return h

    def dev(self, a, role="dev"):
        return self._from(a, np.float32, role)

    def dev_i32(self, a, role="dev_i32"):
        return self._from(a, np.int32, role)

    def dev_i64(self, a, role="dev_i64"):
        return self._from(a, np.int64, role)

    def zeros(self, *shape, role="zeros"):
        return self.full(shape, 0.0, role=role)

    def full(self, shape, v, role="full"):
        h = self._alloc(shape, np.float32, role)
        h[...] = v
        return h

    def bytes_buf(self, nbytes, role="bytes_buf"):
        """exactly nbytes zero bytes (a uint8 handle: read it back with raw())"""
        h = self._alloc((int(nbytes),), np.uint8, role)
        h[...] = 0
        return h

    def sub(self, h, start, stop):
        """h[start:stop] of a flat buffer; the block stays registered while the slice lives"""
        return h[start:stop]

    def ptr(self, h):
        return None if h is None else h.ctypes.data_as(ctypes.c_void_p)

    def np(self, h):
        self.check_guards("read-back")
        return np.array(h, dtype=np.float64)

    def raw(self, h):
        """the buffer's bytes, bit for bit"""
        self.check_guards("read-back")
        return np.ascontiguousarray(h).reshape(-1).view(np.uint8).copy()

    def sync(self):
        pass

    # ---- the check ----
    def _guards(self, b):
        raw = b.ref()
        f = b.start
        k = f + GUARD_BYTES + b.nbytes
        return raw[f:f + GUARD_BYTES], raw[k:k + GUARD_BYTES]

    def _block_of(self, h):
        return next(b for b in self.live_blocks() if b.ref() is (h.base if h.base is not None else h))

    def poke(self, h, offset, flip=0x01):
        """SELF-TEST ONLY: one host-side byte store (bits `flip` inverted) at payload offset `offset` of handle h's block (inside the block:
        -GUARD_BYTES <= offset < nbytes + GUARD_BYTES)"""
        b = self._block_of(h)
        b.ref()[b.start + GUARD_BYTES + offset] ^= flip

    def check_guards(self, what):
        self.checks += 1
        for b in self.live_blocks():
            front, back = self._guards(b)
            if not (np.array_equal(front, _pattern(b.poison, 0)) and np.array_equal(back, _pattern(b.poison, b.nbytes % 4))):
                self._locate(b, front, back, what)


class HipBackend(_Guarded):
    name = "hip"

    def __init__(self, lib):
        import torch
        self.torch = torch
        self.device = torch.device("cuda:0")
        self._pat = {}
        self._init_guards(lib)

    @property
    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _pattern_dev(self, word, phase):
        key = (word, phase)
        if key not in self._pat:
            self._pat[key] = self.torch.from_numpy(_pattern(word, phase).copy()).to(self.device)
        return self._pat[key]

    # ---- guarded allocation ----
    def _alloc(self, shape, dtype, role):
        torch = self.torch
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        block = torch.empty(2 * GUARD_BYTES + nbytes + 16, dtype=torch.uint8, device=self.device)
        start = (-(block.data_ptr() + GUARD_BYTES)) % 16         # the payload on a 16-byte boundary
        b = self._register(weakref.ref(block), start, nbytes, shape, dtype, role)
        block[start:start + GUARD_BYTES] = self._pattern_dev(b.poison, 0)
        block[start + GUARD_BYTES + nbytes:start + 2 * GUARD_BYTES + nbytes] = self._pattern_dev(b.poison, nbytes % 4)
        h = block[start + GUARD_BYTES:start + GUARD_BYTES + nbytes].view(dtype).view(shape)
        h._guard_block = block            # the block is live (registered, checked) exactly as long as its handle is
        return h

    def _from(self, a, np_dtype, dtype, role):
        a = np.ascontiguousarray(np.asarray(a, dtype=np_dtype))
        h = self._alloc(a.shape, dtype, role)
        h.copy_(self.torch.from_numpy(a))
        return h

    def dev(self, a, role="dev"):
        return self._from(a, np.float32, self.torch.float32, role)

    def dev_i32(self, a, role="dev_i32"):
        return self._from(a, np.int32, self.torch.int32, role)

    def dev_i64(self, a, role="dev_i64"):
        return self._from(a, np.int64, self.torch.int64, role)

    def zeros(self, *shape, role="zeros"):
        return self.full(shape, 0.0, role=role)

    def full(self, shape, v, role="full"):
        h = self._alloc(shape, self.torch.float32, role)
        h.fill_(float(v))
        return h

    def bytes_buf(self, nbytes, role="bytes_buf"):
        """exactly nbytes zero bytes (a uint8 handle: read it back with raw())"""
        h = self._alloc((int(nbytes),), self.torch.uint8, role)
        h.zero_()
        return h

    def sub(self, h, start, stop):
        """h[start:stop] of a flat buffer; the block stays registered while the slice lives"""
        v = h[start:stop]
        v._guard_block = getattr(h, "_guard_block", None)
        return v

    def ptr(self, h):
        return None if h is None else ctypes.c_void_p(h.data_ptr())

    def np(self, h):
        self.check_guards("read-back")
        return h.detach().cpu().numpy().astype(np.float64)

    def raw(self, h):
        """the buffer's bytes, bit for bit"""
        self.check_guards("read-back")
        return h.detach().contiguous().reshape(-1).view(self.torch.uint8).cpu().numpy().copy()

    def sync(self):
        self.torch.cuda.synchronize()

    # ---- the check ----
    def _guards(self, b):
        block = b.ref()
        f = b.start
        k = f + GUARD_BYTES + b.nbytes
        return block[f:f + GUARD_BYTES], block[k:k + GUARD_BYTES]

    def _block_of(self, h):
        return next(b for b in self.live_blocks() if b.ref() is h._guard_block)

    def poke(self, h, offset, flip=0x01):
        """SELF-TEST ONLY: one byte (bits `flip` inverted) written by an ordinary torch indexing op at payload offset `offset` of handle h's
        block (inside the block: -GUARD_BYTES <= offset < nbytes + GUARD_BYTES)"""
        b = self._block_of(h)
        b.ref()[b.start + GUARD_BYTES + offset] ^= flip

    def check_guards(self, what):
        """the comparison runs on the device; one flag comes back (the guards themselves only after a failure)"""
        self.checks += 1
        blocks = self.live_blocks()
        if not blocks:
            return
        flags = []
        for b in blocks:
            front, back = self._guards(b)
            flags.append((front != self._pattern_dev(b.poison, 0)).any())
            flags.append((back != self._pattern_dev(b.poison, b.nbytes % 4)).any())
        if bool(self.torch.stack(flags).any().item()):
            for b in blocks:
                front, back = self._guards(b)
                self._locate(b, front.cpu().numpy(), back.cpu().numpy(), what)
