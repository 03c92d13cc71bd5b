"""Guard bands and poison for the device buffers handed to libssrhip.so (a plain test module, no conftest).

The suite compares values; this module lets a test see WHERE a kernel touches memory.

* ``Guarded.alloc(nbytes, dev)``: the buffer sits inside one larger allocation ``[guard | payload | guard]``, every byte 0xFF
  (NaN as float32 / float64, -1 as int32 / int64).  Each guard is GUARD bytes (64 KiB = sixteen magnitude rows of 1028 floats, a
  multiple of 512 so that the payload keeps torch's base alignment); the payload is exactly the bytes asked for, the byte behind it
  is guard already.  A write outside the payload damages a guard; a read of the payload before it is written yields NaN / -1.
* ``Guarded.route(monkeypatch)``: ``backend._workspace`` and the ``empty`` / ``zeros`` / ``full`` / ``empty_like`` of the ``torch``
  name that ``ssr_eval_amd.backend`` and ``ssr_eval_amd.mel`` see hand out guarded device buffers; everything else of torch is
  passed through.  The product's allocation code is not changed.
* ``Guarded.arena(items, gaps, dtype, dev)``: the signals or images of a batch as views into ONE NaN-filled device tensor, NaN in
  front of the first, between them and behind the last.  Arenas are inputs only: they are never handed out as a guarded buffer.
  ``Guarded.read_in_place()`` tells whether the product built a Ragged batch on an arena's storage, i.e. did not pack it.
* ``Guarded.check()``: synchronises, then asserts that every guard byte handed out since the object was made is still 0xFF (the
  message names the allocation by call site and size, the side, and the first and last damaged byte offset) and that every arena is
  bit-identical to what it held when it was made.
"""
import os
import sys

import numpy as np
import torch

GUARD = 64 * 1024                    # bytes per side: >= 16 rows of 1028 floats, a multiple of 512
GAPS_ODD = (1, 3, 5)                 # elements between items: no item base 16-byte aligned relative to the one before
GAPS_QUAD = (4, 8, 12)               # multiples of four elements
INT_POISON = 0x7F7F                  # what an integer arena (int16 PCM) holds outside its items
ARENA_PAD = 1024                     # poisoned elements in front of the first and behind the last item (at least)
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


def _call_site():
    """file:line (function) of the nearest frame outside this module."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?", "?"
    base = os.path.basename(f.f_code.co_filename)
    return "%s:%d (%s)" % (base, f.f_lineno, f.f_code.co_name), "%s:%s" % (base, f.f_code.co_name)


class _Block:
    __slots__ = ("whole", "nbytes", "site", "fn")

    def __init__(self, whole, nbytes, site, fn):
        self.whole, self.nbytes, self.site, self.fn = whole, nbytes, site, fn

    @property
    def payload(self):
        return self.whole[GUARD:GUARD + self.nbytes]

    def sides(self):
        return (("front", self.whole[:GUARD]), ("back", self.whole[GUARD + self.nbytes:]))


class _TorchProxy:
    """`torch` as the product sees it while routed: device allocations come from the guarded allocator."""

    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        return tuple(int(s) for s in size)

    def _routed(self, kw):
        dev = kw.get("device")
        if dev is None or kw.get("pin_memory") or kw.get("out") is not None:
            return None
        dev = torch.device(dev)
        return dev if dev.type == "cuda" else None

    def empty(self, *size, **kw):
        dev = self._routed(kw)
        shape = self._shape(size)
        if dev is None or int(np.prod(shape, dtype=np.int64)) == 0:        # (an empty tensor has nothing to guard; set_() needs a base tensor)
            return torch.empty(*size, **kw)
        return self._owner.empty(shape, kw.get("dtype") or torch.get_default_dtype(), dev)

    def zeros(self, *size, **kw):
        dev = self._routed(kw)
        shape = self._shape(size)
        if dev is None or int(np.prod(shape, dtype=np.int64)) == 0:
            return torch.zeros(*size, **kw)
        return self._owner.empty(shape, kw.get("dtype") or torch.get_default_dtype(), dev).zero_()

    def full(self, size, fill_value, **kw):
        dev = self._routed(kw)
        shape = self._shape((size,))
        if dev is None or int(np.prod(shape, dtype=np.int64)) == 0:
            return torch.full(size, fill_value, **kw)
        return self._owner.empty(shape, kw.get("dtype") or torch.get_default_dtype(), dev).fill_(fill_value)

    def empty_like(self, t, **kw):
        if not t.is_cuda or t.numel() == 0 or kw:
            return torch.empty_like(t, **kw)
        return self._owner.empty(tuple(t.shape), t.dtype, t.device)


class Guarded:
    def __init__(self):
        self.blocks = []                 # every guarded allocation handed out, kept alive until the object goes
        self.arenas = []                 # (tensor, bit-identical copy, call site)
        self.ragged_storages = set()     # storage addresses of every backend.Ragged built while routed

    # ---- guarded allocations ------------------------------------------------------------------------------------------------
    def _block(self, nbytes, dev):
        nbytes = int(nbytes)
        whole = torch.full((2 * GUARD + nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        site, fn = _call_site()
        b = _Block(whole, nbytes, site, fn)
        self.blocks.append(b)
        return b

    def alloc(self, nbytes, dev):
        """uint8 [nbytes] device tensor between two guards, everything 0xFF."""
        return self._block(nbytes, dev).payload

    def empty(self, shape, dtype, dev):
        shape = tuple(int(s) for s in shape)
        es = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64))
        return self._block(n * es, dev).payload.view(dtype).view(shape)

    def workspace(self, nbytes, dev):
        """backend._workspace's contract (never zero-sized) on a guarded block."""
        return self.alloc(max(int(nbytes), 1), dev)

    def route(self, monkeypatch):
        from ssr_eval_amd import backend, mel
        proxy = _TorchProxy(self)
        monkeypatch.setattr(backend, "_workspace", self.workspace)
        monkeypatch.setattr(backend, "torch", proxy)
        monkeypatch.setattr(mel, "torch", proxy)
        init, seen = backend.Ragged.__init__, self.ragged_storages

        def recording_init(r, data, *a, **kw):
            seen.add(data.untyped_storage().data_ptr())
            init(r, data, *a, **kw)
        monkeypatch.setattr(backend.Ragged, "__init__", recording_init)
        return self

    def read_in_place(self):
        """True when every arena made so far became the buffer of a backend.Ragged as it lies (no packing copy in between)."""
        return all(t.untyped_storage().data_ptr() in self.ragged_storages for t, _, _ in self.arenas)

    # ---- poisoned arenas ----------------------------------------------------------------------------------------------------
    def arena(self, items, gaps=GAPS_ODD, dtype=torch.float32, dev="cuda", lead=None, unit=1):
        """items: host arrays (any shape, flattened in C order).  -> (views, offsets, arena): `views[i]` has item i's shape and lies
        at element offsets[i] of the NaN-filled 1-D `arena`; gap i (cycling through `gaps`, in units of `unit` elements) lies between
        item i and item i + 1, ARENA_PAD + lead elements in front of item 0 (lead: gaps[0] by default, so that an odd placement
        starts off a 16-byte boundary too) and at least ARENA_PAD behind the last item."""
        items = [np.ascontiguousarray(a) for a in items]
        lead = int(gaps[0]) if lead is None else int(lead)
        offs, pos = [], ARENA_PAD + lead
        for i, a in enumerate(items):
            offs.append(pos)
            pos += a.size + int(gaps[i % len(gaps)]) * int(unit)
        t = torch.full((pos + ARENA_PAD,), float("nan") if dtype.is_floating_point else INT_POISON, dtype=dtype, device=dev)
        views = []
        for a, o in zip(items, offs):
            v = t[o:o + a.size]
            v.copy_(torch.from_numpy(a.reshape(-1)).to(dtype))
            views.append(v.view(a.shape))
        self.arenas.append((t, t.clone(), _call_site()[0]))
        return views, np.asarray(offs, np.int64), t

    # ---- checker ------------------------------------------------------------------------------------------------------------
    def damage(self):
        """[(block, side, first, last)]: damaged guards; offsets count from the guard's first byte."""
        torch.cuda.synchronize()
        found = []
        for b in self.blocks:
            for side, g in b.sides():
                bad = (g != 0xFF).nonzero().flatten()
                if bad.numel():
                    found.append((b, side, int(bad[0]), int(bad[-1])))
        return found

    def check(self):
        lines = []
        for b, side, first, last in self.damage():
            rel = ("%d .. %d bytes behind the payload's end" % (first, last) if side == "back" else
                   "%d .. %d bytes in front of the payload's start" % (GUARD - last, GUARD - first))
            lines.append("%s guard of the %d-byte buffer allocated at %s damaged: guard bytes %d .. %d (%s)"
                         % (side, b.nbytes, b.site, first, last, rel))
        for t, ref, site in self.arenas:
            a, r = t.view(torch.uint8), ref.view(torch.uint8)
            bad = (a != r).nonzero().flatten()
            if bad.numel():
                es = t.element_size()
                lines.append("input arena of %d elements made at %s was written: elements %d .. %d (bytes %d .. %d)"
                             % (t.numel(), site, int(bad[0]) // es, int(bad[-1]) // es, int(bad[0]), int(bad[-1])))
        if lines:
            raise GuardError("\n".join(lines))

    def untouched_payloads(self, written_ok=()):
        """After a call the library refused: every payload still holds only 0xFF, apart from the buffers allocated in the functions
        `written_ok` names as "file.py:function" (descriptor uploads and launches that come before the refused call).  -> the offending blocks' sites."""
        torch.cuda.synchronize()
        return [b.site for b in self.blocks if b.fn not in written_ok and b.nbytes and bool((b.payload != 0xFF).any())]


class Bits(list):
    """What bits() returns: (shape, dtype, raw bytes) per array."""


def bits(x):
    """A result (tensor, ndarray, or nested lists / tuples of them) as a flat Bits list of (shape, dtype, raw bytes)."""
    if isinstance(x, Bits):
        return x
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        return Bits([(x.shape, x.dtype.str, x.tobytes())])
    if isinstance(x, (list, tuple)):
        return Bits(b for v in x for b in bits(v))
    raise TypeError("no bits of %r" % type(x))


def assert_same_bits(plain, guarded, what=""):
    a, b = bits(plain), bits(guarded)
    assert len(a) == len(b), (what, len(a), len(b))
    for i, ((sa, da, ba), (sb, db, bb)) in enumerate(zip(a, b)):
        assert sa == sb and da == db, (what, i, sa, sb, da, db)
        if ba != bb:
            x, y = np.frombuffer(ba, np.uint8), np.frombuffer(bb, np.uint8)
            bad = np.nonzero(x != y)[0]
            va, vb = np.frombuffer(ba, np.dtype(da)), np.frombuffer(bb, np.dtype(db))
            k = int(bad[0]) // np.dtype(da).itemsize
            raise AssertionError("%s: output %d differs between the plain and the guarded run in %d bytes, first at element %d: %r (plain) "
                                 "against %r (guarded)" % (what, i, bad.size, k, va[k], vb[k]))


def routed():
    """True while Guarded.route() is in force."""
    from ssr_eval_amd import backend
    return isinstance(backend.torch, _TorchProxy)


def assert_only_items_written(out, offs, lens, what=""):
    """out: a guarded output [..., total] in the layout of its input (item i at elements offs[i] .. offs[i] + lens[i] of the last
    dimension): everything in front of the first item, between items and behind the last still holds 0xFF."""
    total = int(out.shape[-1])
    outside = torch.ones(total, dtype=torch.bool, device=out.device)
    for o, n in zip(offs, lens):
        outside[int(o):int(o) + int(n)] = False
    rows = out.reshape(-1, total)
    es = out.element_size()
    for k in range(rows.shape[0]):
        raw = rows[k][outside].contiguous().view(torch.uint8)
        bad = (raw != 0xFF).nonzero().flatten()
        if bad.numel():
            where = outside.nonzero().flatten()[bad // es]
            raise GuardError("%s: output row %d was written outside its items: elements %d .. %d" % (what, k, int(where[0]), int(where[-1])))
