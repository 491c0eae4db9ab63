"""Guard bands around caller buffers: does an entry point stay inside the buffers it is given, and does anything outside
them reach a result?

Every GPU test of the suite hands the library the data_ptr() of a whole torch tensor: 512-byte aligned, exactly as large as
stated, with whatever the caching allocator put next to it on either side.  A kernel that stores a few elements past an
output, or loads past an input, passes every oracle comparison.  Here every caller buffer of a call is PLACED inside a
larger allocation of its own,

    [ front guard | skew | payload | back guard ]

with skew 0 or ONE element (4 bytes for float32 / int32, 8 for float64 / int64 / uint64): the payload stays naturally aligned
but is no longer 16-byte aligned, which is what the launchers' "pointer & 15" arms switch on.  The whole allocation is
filled before the payload is written, once with all-ones bytes (NaN as a float, -1 as an integer) and once with a value
that is valid for that buffer's meaning (1.0f, an in-range token id, an in-range row number), so that an over-read shows
whether it turns a result into NaN or merely into another plausible number.  After the call, bit for bit:

    both guards and the skew gap are unchanged; every input payload is unchanged; an output payload that the header says is
    left alone is unchanged; ids stay inside the range their spec names; and the outputs (and the error the call reported)
    of the two fills are identical -- except where the test hands a comparison of its own for a variable summed with float
    atomics.

A guard is a CONDITION of these tests, not a knob: guard_bytes() takes the payload rounded up to the largest tile the entry
point pads to and never returns less than 64 KiB, so whatever the padding arithmetic of a kernel could overrun stays inside
the test's own allocation -- a defect shows as a changed guard word, never as a fault.

The module works over a small buffer backend (NumpyBackend, TorchBackend): tests/test_guard_bands_host.py proves on the CPU,
with a numpy fake entry point and planted defects, that each of these checks can fail."""
import collections

import numpy as np

MIN_GUARD = 64 << 10
ALIGN = 512                                        # torch's allocator hands out 512-byte aligned blocks; numpy is aligned here
FILLS = ("ones", "valid")
KINDS = ("front guard", "skew gap", "back guard", "input payload", "untouched region", "id out of range", "fill dependence")


class GuardViolation(AssertionError):
    """A check of this module failed; .kind is one of KINDS, .buffer the name of the buffer."""

    def __init__(self, kind, buffer, detail):
        assert kind in KINDS
        AssertionError.__init__(self, "%s: %s -- %s" % (buffer, kind, detail))
        self.kind, self.buffer = kind, buffer


def round_up(n, m):
    return (int(n) + m - 1) // m * m


def guard_bytes(rows, cols, itemsize, tile_rows=64, tile_cols=64):
    """Width of each guard: the payload [rows][cols] rounded up to whole tiles (the largest the entry point pads to), at
    least 64 KiB, a multiple of the allocator's alignment."""
    padded = round_up(max(rows, 1), tile_rows) * round_up(max(cols, 1), tile_cols) * itemsize
    return round_up(max(padded, MIN_GUARD), ALIGN)


# role "in": payload = init, must come back unchanged.  "out": payload starts as the fill and is returned.  "untouched": an
# output the header says this call leaves alone: starts as the fill and must come back as it.
# valid: the value of the second fill (default 1 for floats; integers must name theirs).  id_range = (lo, hi, extra values
# allowed): checked on the payload of an "out" buffer after the call.
Spec = collections.namedtuple("Spec", "dtype n role init valid guard id_range")


def spec(dtype, n, role, init=None, valid=None, guard=None, id_range=None, rows=None, cols=None, tile_rows=64, tile_cols=64):
    dtype = np.dtype(dtype)
    assert role in ("in", "out", "untouched") and (role == "in") == (init is not None)
    if valid is None:
        assert dtype.kind == "f", "an integer buffer names its valid fill value"
        valid = 1.0
    if guard is None:
        guard = guard_bytes(rows if rows is not None else 1, cols if cols is not None else n, dtype.itemsize, tile_rows, tile_cols)
    assert guard >= MIN_GUARD and guard % ALIGN == 0 and guard >= n * dtype.itemsize, "a guard holds at least the payload"
    if init is not None:
        init = np.ascontiguousarray(init, dtype).reshape(-1)
        assert init.size == n
    return Spec(dtype, int(n), role, init, valid, int(guard), id_range)


class NumpyBackend(object):
    """Host memory; a buffer is a uint8 array whose first byte is ALIGN-aligned."""
    name = "numpy"

    def alloc(self, nbytes):
        raw = np.zeros(nbytes + ALIGN, np.uint8)
        off = (-raw.ctypes.data) % ALIGN
        return raw[off:off + nbytes]

    def upload(self, buf, image):
        buf[:] = image

    def download(self, buf):
        return buf.copy()

    def address(self, buf):
        return buf.ctypes.data

    def sync(self):
        pass


class TorchBackend(object):
    """Device memory; a buffer is a uint8 torch tensor of its own (the caching allocator aligns it to 512 bytes)."""
    name = "torch"

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.device = torch, torch.device(device)

    def alloc(self, nbytes):
        t = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
        assert t.data_ptr() % ALIGN == 0
        return t

    def upload(self, buf, image):
        buf.copy_(self.torch.from_numpy(image))

    def download(self, buf):
        self.sync()
        return buf.cpu().numpy()

    def address(self, buf):
        return buf.data_ptr()

    def sync(self):
        self.torch.cuda.synchronize(self.device)


class Guarded(object):
    """One placed buffer.  .ptr is the payload's address; .buf / .offset the allocation and the payload's byte offset."""

    def __init__(self, backend, name, sp, skew, fill):
        assert skew in (0, 1) and fill in FILLS
        self.be, self.name, self.spec, self.skew, self.fill = backend, name, sp, skew, fill
        item = sp.dtype.itemsize
        self.offset = sp.guard + skew * item
        self.nbytes = sp.n * item
        total = round_up(self.offset + self.nbytes + sp.guard, ALIGN)
        cells = np.empty(total // item, sp.dtype)
        if fill == "ones":
            cells.view(np.uint8)[:] = 0xFF
        else:
            cells[:] = sp.valid
        self.prefill = cells.view(np.uint8).copy()             # the whole allocation before the payload is written
        if sp.role == "in":
            cells[self.offset // item:self.offset // item + sp.n] = sp.init
        self.image = cells.view(np.uint8)
        self.buf = backend.alloc(total)
        backend.upload(self.buf, self.image)
        self.ptr = backend.address(self.buf) + self.offset
        assert self.ptr % item == 0 and (self.ptr % 16 == 0) == (skew == 0)

    def tensor(self):
        """The payload as a torch tensor view of the spec's dtype (TorchBackend only): what train_bind_arena takes."""
        t = self.be.torch
        dt = {"float32": t.float32, "int32": t.int32, "float64": t.float64, "int64": t.int64}[self.spec.dtype.name]
        return self.buf[self.offset:self.offset + self.nbytes].view(dt)

    def _first_diff(self, got, want, base):
        bad = np.flatnonzero(got != want)
        item = self.spec.dtype.itemsize
        first, last = int(bad[0]) + base, int(bad[-1]) + base
        return ("%d byte(s) changed, first at element %d, last at element %d relative to the payload start (payload: %d "
                "elements, skew %d, fill %s)" % (bad.size, (first - self.offset) // item, (last - self.offset) // item,
                                                 self.spec.n, self.skew, self.fill))

    def verify(self):
        """Raises GuardViolation for the first of: front guard, skew gap, back guard, input payload, untouched region, id
        range.  Returns the payload (a copy, in the spec's dtype)."""
        now = self.be.download(self.buf)
        sp, g, end = self.spec, self.spec.guard, self.offset + self.nbytes
        for kind, lo, hi in (("front guard", 0, g), ("skew gap", g, self.offset), ("back guard", end, now.size)):
            if not np.array_equal(now[lo:hi], self.image[lo:hi]):
                raise GuardViolation(kind, self.name, self._first_diff(now[lo:hi], self.image[lo:hi], lo))
        if sp.role in ("in", "untouched") and not np.array_equal(now[self.offset:end], self.image[self.offset:end]):
            raise GuardViolation("input payload" if sp.role == "in" else "untouched region", self.name,
                                 self._first_diff(now[self.offset:end], self.image[self.offset:end], self.offset))
        payload = now[self.offset:end].copy().view(sp.dtype)
        if sp.id_range is not None and sp.role == "out":
            lo, hi, extra = sp.id_range
            ok = (payload >= lo) & (payload < hi)
            for v in extra:
                ok |= payload == v
            if not ok.all():
                i = int(np.flatnonzero(~ok)[0])
                raise GuardViolation("id out of range", self.name, "element %d is %r, outside [%d, %d) and %r (skew %d, fill %s)"
                                     % (i, payload[i], lo, hi, tuple(extra), self.skew, self.fill))
        return payload


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.size else a.reshape(-1).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def run_guarded(backend, specs, call, skew, compare=None, fills=FILLS):
    """Places every buffer of `specs` ({name: Spec}) with the given skew, once per fill, and runs call(bufs) on each placement
    (bufs: {name: Guarded}; what call returns -- an error flag, an error text, None -- is kept as the call's status).  Every
    buffer is verified after each call; the payloads of the "out" buffers and the status must be bit-identical between the
    fills, except for the names in `compare` ({name: f(name, first, second)}, which asserts its own bar).
    Returns ({name: payload of every "out" / "untouched" buffer}, status) of the first fill; run_guarded.calls counts calls."""
    first = None
    for fill in fills:
        bufs = collections.OrderedDict((name, Guarded(backend, name, sp, skew, fill)) for name, sp in specs.items())
        backend.sync()
        status = call(bufs)
        backend.sync()
        run_guarded.calls += 1
        outs = collections.OrderedDict()
        for name, b in bufs.items():
            payload = b.verify()
            if b.spec.role != "in":
                outs[name] = payload
        if first is None:
            first = (outs, status, fill)
            continue
        if status != first[1]:
            raise GuardViolation("fill dependence", "status", "the call reported %r under fill %s and %r under fill %s (skew %d)"
                                 % (first[1], first[2], status, fill, skew))
        for name, payload in outs.items():
            if specs[name].role == "untouched":
                continue                                       # (each equals its own fill, checked above)
            if compare and name in compare:
                compare[name](name, first[0][name], payload)
            elif not same_bits(first[0][name], payload):
                bad = np.flatnonzero(bits(first[0][name]) != bits(payload)) // specs[name].dtype.itemsize
                raise GuardViolation("fill dependence", name, "%d element(s) differ between fill %s and fill %s, first at %d: %r / %r "
                                     "(skew %d): memory outside the caller's buffers reached the result"
                                     % (np.unique(bad).size, first[2], fill, bad[0], first[0][name][bad[0]], payload[bad[0]], skew))
    return first[0], first[1]


run_guarded.calls = 0


class Plain(object):
    """The same buffer the way the rest of the suite places it: an allocation of its own of exactly the stated size."""

    def __init__(self, backend, name, sp):
        self.be, self.name, self.spec, self.skew, self.fill = backend, name, sp, 0, "ones"
        cells = np.empty(max(sp.n, 1), sp.dtype)
        cells.view(np.uint8)[:] = 0xFF
        if sp.role == "in":
            cells[:sp.n] = sp.init
        self.buf = backend.alloc(cells.nbytes)
        backend.upload(self.buf, cells.view(np.uint8))
        self.offset, self.nbytes = 0, sp.n * sp.dtype.itemsize
        self.ptr = backend.address(self.buf)

    def tensor(self):
        return Guarded.tensor(self)

    def verify(self):
        return self.be.download(self.buf)[:self.nbytes].copy().view(self.spec.dtype)


def run_plain(backend, specs, call):
    """The same call on whole allocations: ({name: payload of every "out" / "untouched" buffer}, status)."""
    bufs = collections.OrderedDict((name, Plain(backend, name, sp)) for name, sp in specs.items())
    backend.sync()
    status = call(bufs)
    backend.sync()
    return collections.OrderedDict((n, b.verify()) for n, b in bufs.items() if b.spec.role != "in"), status


def drive(backend, specs, call, skew, check=None, compare=None, identical=True):
    """A call as the GPU tests make it: on whole allocations, then guarded under both fills; `check(outs)` holds the guarded
    result to its reference, and (identical) every "out" payload outside `compare` is bit-identical to the whole-allocation
    call's.  Returns the guarded outputs."""
    plain, pstatus = run_plain(backend, specs, call)
    outs, status = run_guarded(backend, specs, call, skew, compare=compare)
    assert status == pstatus, "status %r guarded, %r on whole allocations" % (status, pstatus)
    if check is not None:
        check(outs)
    for name, payload in outs.items():
        if specs[name].role != "out":
            continue
        if compare and name in compare:
            compare[name](name, plain[name], payload)
        elif identical:
            assert same_bits(plain[name], payload), "%s: the guarded call (skew %d) and the whole-allocation call differ in %d elements" % (
                name, skew, int((bits(plain[name]) != bits(payload)).reshape(-1, specs[name].dtype.itemsize).any(axis=1).sum()))
    return outs
