"""A guarded arena for containment tests: where does a kernel read and write?

One uint8 allocation, every byte 0xFF (a NaN in bf16, fp16, fp32 and fp64, non-zero in every integer type), from which named slots are
carved.  Every slot has a guard of its own in front and one behind, each at least GUARD bytes (1 MiB: the one escape this project has
had reached 61 456 bytes), so an access a little outside an operand stays inside memory the test owns: nothing here relies on a fault.

  put(host)       an input: the tensor's bytes in a slot, its neighbourhood NaN; unchanged() later proves it was only read
  out(shape, ..)  an output: 0xFF everywhere unless `fill` is given -- an element the kernel does not write then fails parity whatever
                  the reference value is (NaN compares false with every bound)
  view(nbytes)    a raw workspace
  seal(t)         an out() slot filled by the test itself becomes an input from here on
  check()         every guard byte still 0xFF: compared on the arena's device, ONE scalar read back; on failure the slot, the side and
                  the first and last offending byte are named
  unchanged(t)    an input slot is bit-identical to what was put
  verify()        check() and unchanged() of every input, one read-back when all is well

What this sees: a store outside an operand (guards), an output element left unwritten (0xFF fill), a read outside an operand whose value
reaches a result (NaN, even through a multiplication by zero).  What it cannot see: a read whose value a select discards.

Alignment: a slot starts at a multiple of `align` that is no multiple of 2 * align -- exactly the alignment asked for, never a stronger
one by accident.  The default is the 256 bytes of ops.Arena, which is what the library's callers give every pointer for which
include/vangan_hip.h states no alignment; a pointer for which it states one (16 bytes for vg_spectral_norm's scratch) is passed
with that.

Helper module (no tests in here); works on a CPU tensor as well (tests/test_guarded_host.py)."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

GUARD = 1 << 20
ALIGN = 256
_WIDE = 4096                # slots start on multiples of this (+ align): any power-of-two `align` up to half of it can be honoured exactly


class GuardError(AssertionError):
    pass


class _Slot:
    __slots__ = ('name', 'start', 'end', 'front', 'back', 'tensor', 'ref', 'kind')

    def __init__(self, name, start, end, front, back, tensor, kind):
        self.name, self.start, self.end, self.front, self.back, self.tensor, self.kind = name, start, end, front, back, tensor, kind
        self.ref = None


def nbytes_of(shape: Sequence[int], dtype: torch.dtype) -> int:
    return int(math.prod(shape)) * torch.empty((), dtype=dtype).element_size()


def slot_cost(nbytes: int, guard: int = GUARD) -> int:
    """Upper bound of the arena bytes one slot of `nbytes` payload takes: both guards and the alignment padding."""
    return nbytes + 2 * guard + 2 * _WIDE


class GuardedArena:
    def __init__(self, nbytes: int, device, guard: int = GUARD):
        assert guard >= 1
        self.guard = int(guard)
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self.buf.fill_(0xFF)
        self.device = self.buf.device
        self.slots: List[_Slot] = []
        self._by_ptr = {}
        self.cursor = 0

    # ---- carving ----------------------------------------------------------------------------------------------------------------
    def _carve(self, nbytes: int, align: int, name: Optional[str], kind: str) -> _Slot:
        assert align >= 1 and align & (align - 1) == 0 and 2 * align <= _WIDE, align
        start = -(-(self.cursor + self.guard) // _WIDE) * _WIDE + align         # a multiple of align, not of 2 * align
        end = start + int(nbytes)
        if end + self.guard > self.buf.numel():
            raise MemoryError('guarded arena exhausted: slot %r needs %d more bytes' % (name, end + self.guard - self.buf.numel()))
        s = _Slot(name or 'slot%d' % len(self.slots), start, end, (self.cursor, start), (end, end + self.guard), None, kind)
        self.cursor = end + self.guard
        self.slots.append(s)
        return s

    def _typed(self, s: _Slot, shape, dtype) -> torch.Tensor:
        t = self.buf[s.start:s.end].view(dtype).view(*shape)
        s.tensor = t
        self._by_ptr[t.data_ptr()] = s
        return t

    def out(self, shape: Sequence[int], dtype: torch.dtype = torch.float32, fill=None, name: Optional[str] = None, align: int = ALIGN) -> torch.Tensor:
        """An output slot.  fill None: every byte stays 0xFF (a 'must be overwritten' output); else the value an accumulator starts from."""
        shape = tuple(int(n) for n in shape)
        t = self._typed(self._carve(nbytes_of(shape, dtype), align, name, 'out'), shape, dtype)
        if fill is not None:
            t.fill_(fill)
        return t

    def put(self, host: torch.Tensor, name: Optional[str] = None, align: int = ALIGN, mutable: bool = False) -> torch.Tensor:
        """An input slot holding `host`'s bytes.  mutable: an in/out operand (a gradient that is accumulated into): not sealed."""
        t = self.out(tuple(host.shape), host.dtype, None, name, align)
        t.copy_(host)
        return t if mutable else self.seal(t)

    def seal(self, t: torch.Tensor) -> torch.Tensor:
        """From here on `t` (returned by out()) is an input: verify() / unchanged() compare it with what it holds now."""
        s = self.slot_of(t)
        s.ref = self.buf[s.start:s.end].clone()
        s.kind = 'in'
        return t

    def view(self, nbytes: int, name: Optional[str] = None, align: int = ALIGN) -> torch.Tensor:
        """A raw workspace slot of exactly nbytes bytes (uint8, all 0xFF)."""
        return self._typed(self._carve(int(nbytes), align, name, 'view'), (int(nbytes),), torch.uint8)

    def slot_of(self, t) -> _Slot:
        if isinstance(t, _Slot):
            return t
        if isinstance(t, str):
            return next(s for s in self.slots if s.name == t)
        return self._by_ptr[t.data_ptr()]

    # ---- checking ---------------------------------------------------------------------------------------------------------------
    def _guard_bad(self):
        """Device scalar: guard bytes that are not 0xFF."""
        bad = torch.zeros((), dtype=torch.int64, device=self.device)
        for s in self.slots:
            for a, b in (s.front, s.back):
                bad = bad + (self.buf[a:b] != 0xFF).sum()
        return bad

    def _input_bad(self, s: _Slot):
        return (self.buf[s.start:s.end] != s.ref).sum()

    def _guard_report(self) -> str:
        lines = []
        for s in self.slots:
            for side, (a, b), origin in (('front', s.front, s.start), ('back', s.back, s.end)):
                idx = torch.nonzero(self.buf[a:b] != 0xFF).view(-1)
                if idx.numel():
                    first, last = a + int(idx[0]), a + int(idx[-1])
                    lines.append('slot %r (%s, bytes [%d, %d) of the arena): %s guard, %d bytes changed, first at %+d, last at %+d relative to the '
                                 "slot's %s (arena offsets %d .. %d)" % (s.name, s.kind, s.start, s.end, side, idx.numel(), first - origin,
                                                                         last - origin, 'first byte' if side == 'front' else 'end', first, last))
        return '\n'.join(lines)

    def _input_report(self, s: _Slot) -> str:
        idx = torch.nonzero(self.buf[s.start:s.end] != s.ref).view(-1)
        return 'input slot %r (%d bytes): %d bytes changed, first at byte %d, last at byte %d' % (
            s.name, s.end - s.start, idx.numel(), int(idx[0]), int(idx[-1]))

    def check(self):
        """Every guard byte must still be 0xFF."""
        if int(self._guard_bad()):
            raise GuardError('guard bytes overwritten:\n' + self._guard_report())

    def unchanged(self, slot):
        """An input slot must be bit-identical to what was put."""
        s = self.slot_of(slot)
        assert s.ref is not None, 'slot %r is no input' % s.name
        if int(self._input_bad(s)):
            raise GuardError(self._input_report(s))

    def verify(self):
        """check() and unchanged() of every input slot; one scalar read back when nothing is wrong."""
        bad = self._guard_bad()
        ins = [s for s in self.slots if s.ref is not None]
        for s in ins:
            bad = bad + self._input_bad(s)
        if int(bad):
            self.check()
            for s in ins:
                self.unchanged(s)
            raise GuardError('verify() counted %d bad bytes but found none on the second look' % int(bad))
