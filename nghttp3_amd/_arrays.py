"""What the state classes of qpack.py share: the host-or-device array backend,
the capacity rule, and the two call sequences built on QH_ERR_NOMEM naming the
exact need (retry once grown; size, allocate, call)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

SENTINEL = 0xA5


def cap_for(need: int, minimum: int) -> int:
    """The smallest minimum * 2**k >= need: every owned array and remembered
    output capacity grows by this rule, so that most calls find room."""
    cap = minimum
    while cap < need:
        cap *= 2
    return cap


def _np_size(a):
    return 0 if a is None else a.size


def _np_ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)


def _t_size(t):
    return 0 if t is None else t.numel()


def _t_ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


class Backend:
    """The arrays of one state object and the calls over them.  Host form
    (device None): numpy arrays and the qh_qpack_<stem> twins.  Device form:
    torch tensors on one device and the qh_<stem>_batch calls, made with the
    context of `codec` (the one given here, or the one given to ``call``)."""

    def __init__(self, device=None, codec=None):
        self.codec = codec
        self.dev = device is not None
        self._nolist = None
        self._fns = {}
        # size(a): 0 for None.  ptr(a): NULL for None and for an empty array, which has no address
        self.size, self.ptr = (_t_size, _t_ptr) if self.dev else (_np_size, _np_ptr)
        if self.dev:
            import torch
            self.torch, self.device = torch, torch.device(device)
            self._dtypes = {np.uint8: torch.uint8, np.int32: torch.int32}

    def zeros(self, n, dtype=np.uint8):
        if self.dev:
            return self.torch.zeros(n, dtype=self._dtypes[dtype], device=self.device)
        return np.zeros(n, dtype=dtype)

    def empty(self, n, dtype=np.uint8):
        """Uninitialised on the device, where zeros would launch a fill kernel
        (numpy's zeroed pages cost nothing, and the host results stay as they
        were)."""
        if self.dev:
            return self.torch.empty(n, dtype=self._dtypes[dtype], device=self.device)
        return np.zeros(n, dtype=dtype)

    def room(self, cap, pad=0, unit=1):
        """A zeroed output of cap (+ pad) units of `unit` bytes; with pad (the
        tests' fixed capacities) sentinel bytes lie behind the given room."""
        a = self.zeros((cap + pad) * unit)
        if pad:
            a[cap * unit:] = SENTINEL
        return a

    def put(self, a):
        """A numpy array as an array of this backend."""
        return self.torch.from_numpy(a).to(self.device) if self.dev else a

    def host(self, a):
        """-> a numpy copy."""
        return a.cpu().numpy() if self.dev else a.copy()

    @staticmethod
    def own(a):
        return a.copy() if isinstance(a, np.ndarray) else a.clone()

    def list_ptr(self, sel):
        """The pointer of a table list.  None stays NULL ("every table" /
        "item p -> table p"); a list that is given but empty is still a list,
        so it points at four bytes nobody reads (its length is 0)."""
        if sel is not None and self.size(sel) == 0:
            if self._nolist is None:
                self._nolist = self.empty(4)
            sel = self._nolist
        return self.ptr(sel)

    def name(self, stem):
        return "qh_%s_batch" % stem if self.dev else "qh_qpack_" + stem

    def call(self, lib, stem, *args, codec=None):
        """qh_qpack_<stem>(args) or qh_<stem>_batch(ctx, args, QH_WHERE_DEVICE)."""
        fn = self._fns.get(stem)
        if fn is None:
            fn = self._fns[stem] = getattr(lib, self.name(stem))
        codec = codec or self.codec
        assert (codec is not None) == self.dev, "a device form takes a codec, a host form none"
        return fn(codec._ctx, *args, _lib.QH_WHERE_DEVICE) if self.dev else fn(*args)

    def check(self, rv, stem):
        _lib.check(rv, self.name(stem))

    def retry(self, stem, attempt, grow, fixed=False, tries=2):
        """attempt() -> (rv, needs).  On QH_ERR_NOMEM the needs are exact:
        grow(needs) enlarges and the call is made once more.  `fixed` (the
        tests' fixed capacities): the call is made once and rv handed back
        unchecked.  The caller advances its state only when rv == 0."""
        for _ in range(tries):
            rv, needs = attempt()
            if rv != _lib.QH_ERR_NOMEM or fixed:
                break
            grow(needs)
        if not fixed:
            self.check(rv, stem)
        return rv, needs

    def sized(self, stem, call, rooms, alloc):
        """A compaction: call(outs) -> (rv, needs) first without outputs (the
        sizing call), then with fresh arrays of cap_for(need, minimum) units
        of `unit` bytes each (rooms: (unit, minimum) per output), so that the
        next growing call finds room.  -> (outs, needs)."""
        rv, needs = call([None] * len(rooms))
        if rv != _lib.QH_ERR_NOMEM:
            self.check(rv, stem)  # (0: nothing to keep; the arrays are still replaced)
        outs = [alloc(cap_for(n, m) * u) for n, (u, m) in zip(needs, rooms)]
        rv, needs = call(outs)
        self.check(rv, stem)
        return outs, needs


def grow(obj, name: str, have: int, need: int, minimum: int):
    """obj.<name> (bytes) enlarged to cap_for(need, at least what it is),
    its first `have` bytes kept."""
    old = getattr(obj, name)
    size = old.size if isinstance(old, np.ndarray) else old.numel()
    if need <= size:
        return
    cap = cap_for(need, max(minimum, size))
    if isinstance(old, np.ndarray):
        new = np.zeros(cap, dtype=np.uint8)
    else:
        import torch
        new = torch.empty(cap, dtype=torch.uint8, device=old.device)
    new[:have] = old[:have]
    setattr(obj, name, new)
