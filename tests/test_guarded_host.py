"""CPU controls of tests/guarded.py: the arena on a host tensor; one flipped byte in a front guard, in a back guard and in an input must
be reported with the right slot, side and offset -- so a green check() on the GPU means something."""
import pytest
import torch

import guarded as G


def _arena():
    ar = G.GuardedArena(16 << 20, 'cpu')
    a = ar.put(torch.arange(1000, dtype=torch.float32), name='a')
    o = ar.out((3, 5, 7), torch.bfloat16, name='o')
    z = ar.out((33,), torch.float32, fill=0.0, name='z')
    w = ar.view(12345, name='w', align=16)
    return ar, a, o, z, w


def test_layout_fill_and_alignment():
    ar, a, o, z, w = _arena()
    assert torch.equal(a, torch.arange(1000, dtype=torch.float32))
    assert bool(torch.isnan(o.float()).all()) and bool((z == 0).all()) and bool((w == 0xFF).all())
    base = ar.buf.data_ptr()
    prev_end = 0
    for s in ar.slots:
        assert s.front == (prev_end, s.start) and s.start - prev_end >= G.GUARD          # a guard of its own in front ...
        assert s.back == (s.end, s.end + G.GUARD)                                        # ... and behind, shared with no neighbour
        prev_end = s.back[1]
        assert s.tensor.data_ptr() == base + s.start
    for t, al in ((a, 256), (o, 256), (z, 256), (w, 16)):
        off = t.data_ptr() - base
        assert off % al == 0 and off % (2 * al) != 0                                     # the alignment asked for, and no stronger one
    for dt in (torch.bfloat16, torch.float16, torch.float32, torch.float64):
        assert bool(torch.isnan(ar.buf[:64].view(dt)).all())
    for dt in (torch.int32, torch.int64, torch.uint8):
        assert bool((ar.buf[:64].view(dt) != 0).all())
    ar.check()
    ar.unchanged(a)
    ar.verify()
    assert G.slot_cost(1000) >= ar.slots[0].back[1]


@pytest.mark.parametrize('where', ['first', 'last', 'both'])
def test_flipped_byte_in_a_front_guard_is_named(where):
    ar, a, o, z, w = _arena()
    s = ar.slot_of(o)
    hits = {'first': [-(s.start - s.front[0])], 'last': [-1], 'both': [-4000, -17]}[where]
    for h in hits:
        ar.buf[s.start + h] = 0
    with pytest.raises(G.GuardError) as e:
        ar.check()
    msg = str(e.value)
    assert "slot 'o'" in msg and 'front guard' in msg and "slot 'a'" not in msg and "slot 'z'" not in msg
    assert '%d bytes changed, first at %+d, last at %+d' % (len(hits), hits[0], hits[-1]) in msg
    with pytest.raises(G.GuardError):
        ar.verify()


def test_flipped_byte_in_a_back_guard_is_named():
    ar, a, o, z, w = _arena()
    s = ar.slot_of(w)
    ar.buf[s.end] = 0xFE                      # the first byte behind a workspace of an odd size
    ar.buf[s.end + 61455] = 0x00
    with pytest.raises(G.GuardError) as e:
        ar.check()
    msg = str(e.value)
    assert "slot 'w'" in msg and 'back guard' in msg and 'front guard' not in msg
    assert '2 bytes changed, first at +0, last at +61455' in msg
    assert 'arena offsets %d .. %d' % (s.end, s.end + 61455) in msg


def test_changed_input_is_named():
    ar, a, o, z, w = _arena()
    ar.buf[ar.slot_of(a).start + 401] ^= 1
    ar.check()                                # the guards are intact
    with pytest.raises(G.GuardError) as e:
        ar.unchanged(a)
    assert "input slot 'a'" in str(e.value) and 'first at byte 401, last at byte 401' in str(e.value)
    with pytest.raises(G.GuardError) as e:
        ar.verify()
    assert "input slot 'a'" in str(e.value)
    with pytest.raises(AssertionError):
        ar.unchanged(o)                       # an output is no input


def test_seal_and_mutable():
    ar = G.GuardedArena(8 << 20, 'cpu')
    t = ar.out((10,), torch.float32, fill=0.0, name='t')
    t[3] = 2.0
    ar.seal(t)
    m = ar.put(torch.ones(4), name='m', mutable=True)
    m += 1                                    # an accumulated-into operand may change
    ar.verify()
    t[3] = 3.0
    with pytest.raises(G.GuardError):
        ar.verify()


def test_exhaustion_is_an_error():
    ar = G.GuardedArena(3 << 20, 'cpu')
    ar.out((16,), torch.float32)
    with pytest.raises(MemoryError):
        ar.out((16,), torch.float32)
