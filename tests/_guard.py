"""Guard bands around device buffers, and read-only inputs: what a kernel writes OUTSIDE the region it was given.

The parity suites compare what a kernel was asked to write.  A 16-byte store over a ragged tail, a last tile one row too far, the
word in front of `y` or a scribble into `x` lands in the slack of torch's caching allocator (512-byte-rounded blocks inside large
segments): no fault, no difference.  Here every buffer is the middle of its own `uint8` allocation

    [ G bytes | off bytes | nbytes: the typed view the kernel gets | G bytes ]

filled with the byte `SENTINEL`.  G = 512, so the view has the base alignment of a torch allocation (the launchers test bases
against 16 and 64) unless `off` asks for less.  `SENTINEL` = 0xA5: as i32 it is -1515870811 (neither 0 nor the suites' -77 poison),
as f32 -2.87e-16 and as f64 -1.2e-129 (no NaN, no zero), so a kernel that copies its own poison or zeros into a band is seen.

`Guards.check(op)` compares, in ONE device comparison and one synchronisation, both bands of every buffer with the sentinel and
every buffer uploaded `readonly=True` with the copy taken at upload, bands included (an input above 1 MiB is compared on its own,
to spare a second copy of it).  On a difference it downloads the buffers and raises `GuardError` (an AssertionError) naming the op,
the buffer's role, the side and the byte offset of the first changed byte relative to the start of the valid region: negative in
front of it, >= nbytes behind it.

Run time: nobody has measured it yet.  The issue accepts up to 1.5x the parent's wall time for `pytest tests/test_gpu_parity.py -m gpu`
and for the whole `-m gpu` run on one machine; what a call adds is one fill per buffer, one copy per read-only input and the
comparison above (two concatenations, one `torch.equal`).

Test infrastructure only."""
from __future__ import annotations

import numpy as np

SENTINEL = 0xA5
G = 512  # bytes per band; a multiple of 512 keeps torch's base alignment for the view


class GuardError(AssertionError):
    pass


class Buffer:
    """One guarded device buffer: `t` is the typed 1-D view of `nelem` elements that starts `G + off` bytes into `raw`."""

    def __init__(self, role, nelem, dtype, off=0, device="cuda:0"):
        import torch

        item = torch.empty(0, dtype=dtype).element_size()
        assert off >= 0 and off % item == 0, "the view must stay aligned to its element"
        self.role, self.nbytes = role, int(nelem) * item
        self.lo, self.hi = G + off, G + off + self.nbytes
        self.raw = torch.full((self.hi + G,), SENTINEL, dtype=torch.uint8, device=device)
        self.t = self.raw[self.lo:self.hi].view(dtype)
        self.frozen = None  # a copy of `raw` from the moment the content became read-only

    def freeze(self):
        self.frozen = self.raw.clone()

    def first_change(self):
        """(side, byte offset relative to the valid region) of the first changed byte, or None.  Host side, failure path only."""
        raw = self.raw.cpu().numpy()
        want = np.full_like(raw, SENTINEL) if self.frozen is None else self.frozen.cpu().numpy()
        if self.frozen is None:
            want[self.lo:self.hi] = raw[self.lo:self.hi]
        bad = np.flatnonzero(raw != want)
        if bad.size == 0:
            return None
        at = int(bad[0])
        return ("before" if at < self.lo else "after" if at >= self.hi else "inside"), at - self.lo


class Guards:
    """The guarded buffers of one engine call (or of a few consecutive ones that share a state)."""

    def __init__(self, device="cuda:0"):
        self.device = device
        self.bufs = []

    def empty(self, role, nelem, dtype, off=0):
        """`nelem` elements of `dtype`, content = sentinel bytes; `off`: bytes between the allocation's 512-byte grid and the view."""
        b = Buffer(role, nelem, dtype, off, self.device)
        self.bufs.append(b)
        return b.t

    def full(self, role, nelem, dtype, fill, off=0):
        t = self.empty(role, nelem, dtype, off)
        t.fill_(fill)
        return t

    def upload(self, role, a, off=0, readonly=False):
        """numpy -> device, same shape (uint32 travels as int32).  readonly: `check` holds the content to what was uploaded."""
        import torch

        a = np.ascontiguousarray(a)
        host = torch.from_numpy((a.view(np.int32) if a.dtype == np.uint32 else a).copy())
        t = self.empty(role, host.numel(), host.dtype, off)
        t.copy_(host.reshape(-1))
        if readonly:
            self.bufs[-1].freeze()
        return t.reshape(host.shape)

    def freeze(self, role):
        """The buffer last created with `role` is read-only from here on (bands and content as they are now)."""
        [b for b in self.bufs if b.role == role][-1].freeze()

    def check(self, op):
        """Call after the engine call AND torch.cuda.synchronize().  One device comparison for all buffers."""
        import torch

        if not self.bufs:
            return
        cur, want = [], []
        sent = _sentinels(self.device, max(b.lo for b in self.bufs))
        same = True
        for b in self.bufs:
            if b.frozen is not None and b.raw.numel() > _FOLD_MAX:
                same = same and torch.equal(b.raw, b.frozen)  # no second copy of a large input just to fold the comparison
            elif b.frozen is not None:
                cur.append(b.raw), want.append(b.frozen)
            else:
                cur += [b.raw[:b.lo], b.raw[b.hi:]]
                want += [sent[:b.lo], sent[:G]]
        if same and (not cur or torch.equal(torch.cat(cur), torch.cat(want))):
            return
        for b in self.bufs:
            hit = b.first_change()
            if hit is not None:
                side, at = hit
                what = "read-only input modified" if side == "inside" else f"stray write {side} the buffer"
                raise GuardError(f"{op}: `{b.role}`: {what}, first changed byte at offset {at:+d} relative to the valid region "
                                 f"of {b.nbytes} bytes ({side})")
        raise GuardError(f"{op}: the device comparison failed but no changed byte was found")


_FOLD_MAX = 1 << 20  # read-only buffers up to this many bytes join the one folded comparison
_SENT = {}


def _sentinels(device, n):
    import torch

    t = _SENT.get(str(device))
    if t is None or t.numel() < n:
        t = _SENT[str(device)] = torch.full((max(n, G + 64),), SENTINEL, dtype=torch.uint8, device=device)
    return t
