"""Guard bands around every tensor the library allocates or is handed: where the kernels read and write, not what they compute.

The C entries see raw pointers, and torch's caching allocator hides both kinds of mistake: a store past the end of an output lands in some other live
block, and an output element that is never stored still holds the right answer from the previous call.  Here every allocation of the library becomes
the middle of a private arena

    [ 4096 guard bytes | payload, poisoned with 0xFF | 4096 guard bytes ]

whose tail guard starts at the payload's last byte.  0xFF.. is a NaN in float32, bfloat16 and float16 alike, so an element nobody stored shows; the
guards are 0xA5 (or, around an input, a byte the test chooses -- 0x00 in one run and 0xFF in the next, so a read past an input changes the result).
4096 is a multiple of every alignment the kernels assume: the payload keeps the alignment the allocator gave.

Five properties, checked by run_properties for one call of the library:
  A  nothing outside an allocation is written           (all guards intact after the call)
  B  everything inside an output is written             (poisoned call == plain call, no NaN)
  C  nothing outside an input is read into the result   (guards of the inputs 0x00 vs 0xFF: same result, no NaN)
  D  inputs are not modified                            (payload and guards of every input byte-identical afterwards)
  E  the promised workspace is enough                   (every workspace is exactly as large as its *_bytes query says; A and B then hold)

Not a conftest and not a plugin: a plain module the tests import.
"""
import contextlib
import importlib
import sys

import torch

GUARD = 4096
GUARD_BYTE = 0xA5
POISON = 0xFF

# the modules of the library that allocate: each one's own `torch` name is replaced for the duration of guarded_library()
LIBRARY_MODULES = ("recnext_amd.ops", "recnext_amd.recconv", "recnext_amd.dwconv", "recnext_amd.recattn", "recnext_amd.lsmodels", "recnext_amd.layers")


class Arena:
    """One guarded allocation: buf = guard + payload + guard (uint8), tensor = the view of the payload handed out."""

    def __init__(self, order, kind, label, buf, nbytes, tensor, fill):
        self.order, self.kind, self.label, self.buf, self.nbytes, self.tensor, self.fill = order, kind, label, buf, nbytes, tensor, fill
        self.snapshot = None

    def describe(self):
        return f"{self.kind} #{self.order} ({self.label}) shape {tuple(self.tensor.shape)} {self.tensor.dtype}, {self.nbytes} bytes"


def _span(shape, strides):
    """Elements of storage a (shape, strides) view reaches from its first element: 0 for an empty tensor."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


def _arena(shape, strides, dtype, device, fill, poison, order, kind, label):
    itemsize = torch.empty((), dtype=dtype).element_size()
    nbytes = _span(shape, strides) * itemsize
    buf = torch.empty(2 * GUARD + nbytes, dtype=torch.uint8, device=device)
    buf[:GUARD].fill_(fill)
    buf[GUARD + nbytes:].fill_(fill)                       # the tail guard starts at the payload's last byte: an overrun of one element lands in it
    if poison is not None:
        buf[GUARD:GUARD + nbytes].fill_(poison)
    view = buf[GUARD:GUARD + nbytes].view(dtype).as_strided(tuple(shape), tuple(strides))
    return Arena(order, kind, label, buf, nbytes, view, fill)


def _caller(depth=2):
    """'function:line < function:line' of the library code that asked for the allocation."""
    out = []
    f = sys._getframe(depth)
    while f is not None and len(out) < 2:
        out.append(f"{f.f_code.co_name}:{f.f_lineno}")
        f = f.f_back
    return " < ".join(out)


class _TorchProxy:
    """Stands in for a module's `torch` name: everything is the real torch's, except empty and empty_like."""

    def __init__(self, recorder):
        self.__dict__["_rec"] = recorder

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        meta = torch.empty(*size, dtype=dtype, device="meta", **kw)             # shape, dtype and strides as the real call would make them
        device = torch.empty(0, device=device).device if device is None else torch.device(device)
        return self._rec.allocate(meta.shape, meta.stride(), meta.dtype, device, "empty", _caller())

    def empty_like(self, t, *, dtype=None, device=None, **kw):
        like = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="meta")
        meta = torch.empty_like(like, dtype=dtype, **kw)
        return self._rec.allocate(meta.shape, meta.stride(), meta.dtype, t.device if device is None else torch.device(device), "empty_like", _caller())


class Recorder:
    def __init__(self):
        self.arenas = []
        self.proxy = _TorchProxy(self)

    def allocate(self, shape, strides, dtype, device, kind, label):
        a = _arena(shape, strides, dtype, device, GUARD_BYTE, POISON, len(self.arenas), kind, label)
        self.arenas.append(a)
        return a.tensor


@contextlib.contextmanager
def guarded_library(modules=None):
    """Every torch.empty / torch.empty_like of the library's allocating modules (or of `modules`) comes out of a poisoned, guarded arena; yields the
    Recorder whose .arenas lists them in call order.  torch itself is not touched: only each module's own `torch` global."""
    mods = [importlib.import_module(m) if isinstance(m, str) else m for m in (LIBRARY_MODULES if modules is None else modules)]
    rec = Recorder()
    saved = []
    try:
        for m in mods:
            if getattr(m, "torch", None) is torch:
                saved.append(m)
                m.torch = rec.proxy
        yield rec
    finally:
        for m in saved:
            m.torch = torch


def guarded_copy(t, fill, arenas=None):
    """A copy of input tensor t in an arena of its own, same shape, dtype and strides, the guards filled with `fill`.  The arena (with a snapshot of all
    its bytes, for check_inputs_unchanged) is appended to `arenas`."""
    order = len(arenas) if arenas is not None else 0
    a = _arena(t.shape, t.stride(), t.dtype, t.device, fill, fill, order, "input", _caller())      # gaps of a non-dense input hold `fill` too
    a.tensor.copy_(t.detach())
    a.snapshot = a.buf.clone()
    if arenas is not None:
        arenas.append(a)
    return a.tensor


def check_guards(arenas):
    """Property A: every guard byte of every arena still holds its fill.  Names the first arena that does not."""
    arenas = list(arenas)
    if not arenas:
        return
    flags = torch.stack([(torch.cat([a.buf[:GUARD], a.buf[GUARD + a.nbytes:]]) != a.fill).any() for a in arenas]).cpu()      # one read-back for all
    for a, bad in zip(arenas, flags.tolist()):
        if not bad:
            continue
        head = (a.buf[:GUARD] != a.fill).nonzero().flatten().cpu()
        tail = (a.buf[GUARD + a.nbytes:] != a.fill).nonzero().flatten().cpu()
        first = int(head[0]) - GUARD if len(head) else a.nbytes + int(tail[0])
        raise AssertionError(f"guard band overwritten: {a.describe()}: first changed byte at offset {first} relative to the payload "
                             f"({len(head)} bytes changed in front of it, {len(tail)} behind it)")


def check_inputs_unchanged(arenas):
    """Property D: payload and guards of every guarded_copy are byte-identical to what they were when it was made."""
    for a in arenas:
        if a.snapshot is None:
            continue
        diff = (a.buf != a.snapshot).nonzero().flatten().cpu()
        if len(diff):
            raise AssertionError(f"input modified: {a.describe()}: first changed byte at offset {int(diff[0]) - GUARD} relative to the payload "
                                 f"({len(diff)} bytes changed)")


def _tensors(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _tensors(o)]
    return []


def check_written(out, what="result"):
    """No floating-point element of a result is NaN: the 0xFF poison of an unwritten element, or of unwritten scratch that fed it, is one."""
    for i, t in enumerate(_tensors(out)):
        if t.is_floating_point() and t.numel():
            nan = torch.isnan(t)
            if bool(nan.any()):
                idx = nan.nonzero()[0].tolist()
                raise AssertionError(f"{what} {i} (shape {tuple(t.shape)} {t.dtype}) holds {int(nan.sum())} NaN elements, the first at {tuple(idx)}: "
                                     "an element nobody stored, or scratch read before it was written")


def check_same(got, want, what, same=None):
    """The floating-point tensors of two results agree: torch.equal unless the case brings its own bar `same(got, want)` (raw byte buffers such as the
    saved pyramid are not compared: their padding is nobody's output)."""
    got, want = _tensors(got), _tensors(want)
    assert len(got) == len(want), f"{what}: {len(got)} tensors against {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and g.stride() == w.stride(), f"{what}: tensor {i} is {tuple(g.shape)} {g.dtype} {g.stride()}, expected {tuple(w.shape)} {w.dtype} {w.stride()}"
        if not g.is_floating_point():
            continue
        ok = torch.equal(g, w) if same is None else same(g, w)
        if not ok:
            d = (g.float() - w.float()).abs()
            raise AssertionError(f"{what}: tensor {i} (shape {tuple(g.shape)} {g.dtype}) differs in {int((g != w).sum())} elements, max |diff| {float(d.nan_to_num(float('inf')).max()):.3e}")


def map_tensors(args, fn, memo=None):
    """args with every tensor replaced by fn(tensor); one tensor passed twice stays one tensor (the aliased calls)."""
    memo = {} if memo is None else memo
    if torch.is_tensor(args):
        if id(args) not in memo:
            memo[id(args)] = fn(args)
        return memo[id(args)]
    if isinstance(args, (tuple, list)):
        return type(args)(map_tensors(a, fn, memo) for a in args)
    if isinstance(args, dict):
        return {k: map_tensors(v, fn, memo) for k, v in args.items()}
    return args


def _sync(args):
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def run_properties(invoke, args, same=None, modules=None, repeat=True):
    """Properties A - D for result = invoke(*args): args a tuple of tensors, None, numbers and (nested) lists of them; the result a tensor or a tuple.
    `same`: None for an entry whose repeat launches are bit-identical (asserted here first), else the bar of its own parity test.  Returns the plain result."""
    plain = invoke(*args)
    if repeat:
        check_same(invoke(*args), plain, "repeat launch", same)
    check_written(plain, "plain result")
    # A + B: the library's own allocations poisoned and guarded
    with guarded_library(modules) as rec:
        poisoned = invoke(*args)
        _sync(args)
        check_guards(rec.arenas)
    check_written(poisoned, "poisoned result")
    check_same(poisoned, plain, "poisoned allocations against the plain call", same)
    # C + D (and A again): every input in an arena of its own, guards 0x00 then 0xFF
    results = []
    for fill in (0x00, 0xFF):
        inputs = []
        gargs = map_tensors(args, lambda t: guarded_copy(t, fill, inputs))
        with guarded_library(modules) as rec:
            out = invoke(*gargs)
            _sync(args)
            check_guards(rec.arenas + inputs)
        check_inputs_unchanged(inputs)
        check_written(out, f"result with input guards {fill:#04x}")
        results.append(out)
    check_same(results[0], results[1], "input guards 0x00 against 0xFF", same)
    check_same(results[0], plain, "guarded inputs against the plain call", same)
    return plain
