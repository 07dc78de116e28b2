"""Guarded buffers for the C ABI (include/dfgnn.h): every array a call sees lives in the middle of a larger buffer the test
owns, so that a store past an output's end, a slot a kernel never writes, a modified input and a load past an input's end
that reaches an output all become assertion failures instead of silent luck (tests/test_gpu_guarded.py; the helper's own
test, on CPU tensors, is tests/test_guarded_host.py).

    arena = Arena(device)                      # shift=1: every float view starts one float after a 16-byte boundary
    q   = arena.input("Q", Q)                  # a copy of Q between guards
    out = arena.output("out", (m, h, f))       # NaN-filled view between NaN-filled guards
    ws  = arena.scratch("ws", n, aligned=True) # as an output, contents unconstrained; aligned: 16-byte aligned under shift
    ... call the entry with q.data_ptr(), out.data_ptr(), ws.data_ptr() ...
    arena.verify()                             # or verify(outputs=[...], scratch=[...], inputs=[...]) by name

The fill.  Float buffers -- guards and the views of outputs and scratch -- hold ONE quiet NaN with a distinctive payload
(FILL_BITS); it is written and compared through an int32 view, so a NaN that a kernel computes (0x7fc00000, or an operand's
payload carried through) is never mistaken for it.  Integer outputs hold INT_FILL, a negative number no index, offset or
count equals.  The guards of INTEGER INPUTS hold 0: an index that leaks out of a guard gathers row 0, never an address out of
bounds.  Every guard has at least GUARD elements on each side.

verify asserts, naming the buffer and the first offending offset relative to the view's start:
  * every guard of every recorded buffer is bit-identical to its fill;
  * no element of an output still carries the fill, and every float output element is finite (the operators' sentinels,
    row_max = -1e38, are finite; the header allows no inf or NaN in any output);
  * every input view is bit-identical to what was copied in;
  * nothing about the contents of scratch.

What this cannot see: a load past an input's end whose value never reaches an output."""
import re

import numpy as np
import torch

GUARD = 1 << 16
FILL_BITS = 0x7FC5A5A5                      # a quiet NaN, payload 0x5a5a5: no arithmetic produces it
INT_FILL = -0x5A5A5A5B                      # int32 outputs (0xa5a5a5a5): no id, offset or count is negative
_INT_BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int16: torch.int16, torch.int64: torch.int64,
             torch.uint8: torch.uint8}
_BYTE_FILL = 0xA5


class _Record:
    __slots__ = ("name", "kind", "buf", "view", "lo", "n", "fill", "guard_fill", "snapshot")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _first(mask):
    return int(torch.nonzero(mask.reshape(-1))[0])


class Arena:
    def __init__(self, device, shift=0, guard=GUARD):
        assert shift in (0, 1) and guard >= GUARD
        self.device, self.shift, self.guard = torch.device(device), shift, guard
        self.records = {}

    # ---- allocation ---------------------------------------------------------------------------------------------------
    def _make(self, name, kind, shape, dtype, fill, guard_fill, aligned):
        assert name not in self.records, f"{name}: recorded twice"
        assert dtype in _INT_BITS, dtype
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        esize = torch.empty((), dtype=dtype).element_size()
        g = self.guard * (4 // esize if esize < 4 else 1)              # at least GUARD elements, a multiple of 16 bytes
        lo = g + (self.shift if dtype == torch.float32 and not aligned else 0)
        buf = torch.empty(lo + n + g, dtype=dtype, device=self.device)
        bits = _bits(buf)
        bits[:lo] = guard_fill
        bits[lo + n:] = guard_fill
        bits[lo:lo + n] = fill
        r = _Record()
        r.name, r.kind, r.buf, r.lo, r.n, r.fill, r.guard_fill, r.snapshot = name, kind, buf, lo, n, fill, guard_fill, None
        r.view = buf[lo:lo + n].view(shape)
        want = 4 if (self.shift and dtype == torch.float32 and not aligned) else 0
        assert r.view.data_ptr() % 16 == want, (name, r.view.data_ptr() % 16, want)
        assert r.view.is_contiguous()
        self.records[name] = r
        return r

    def output(self, name, shape, dtype=torch.float32, aligned=False):
        """A view the call must write in full.  float32: NaN fill; int32: INT_FILL."""
        assert dtype in (torch.float32, torch.int32)
        fill = FILL_BITS if dtype == torch.float32 else INT_FILL
        return self._make(name, "output", shape, dtype, fill, fill, aligned).view

    def scratch(self, name, numel, dtype=torch.float32, aligned=False):
        """Workspace of exactly `numel` elements: guards checked, contents unconstrained."""
        fill = {torch.float32: FILL_BITS, torch.int32: INT_FILL, torch.uint8: _BYTE_FILL}[dtype]
        return self._make(name, "scratch", (numel,), dtype, fill, fill, aligned).view

    def input(self, name, value, aligned=False):
        """A copy of `value` (numpy array or tensor) between guards: NaN guards for float32, zero guards for integers."""
        t = torch.as_tensor(np.ascontiguousarray(value) if isinstance(value, np.ndarray) else value)
        fill = FILL_BITS if t.dtype == torch.float32 else 0
        r = self._make(name, "input", t.shape, t.dtype, fill, fill, aligned)
        r.view.copy_(t.to(self.device))
        r.snapshot = _bits(r.view).clone()
        return r.view

    def __getitem__(self, name):
        return self.records[name].view

    def __len__(self):
        return len(self.records)

    # ---- the check ----------------------------------------------------------------------------------------------------
    def _names(self, kind, names):
        if names is None:
            return [r.name for r in self.records.values() if r.kind == kind]
        names = list(names)
        for n in names:
            assert self.records[n].kind == kind, f"{n} is recorded as {self.records[n].kind}, not as {kind}"
        return names

    def _suspect(self, outputs, inputs):
        """Whether any check of verify would fire: the same comparisons reduced on the device and read back once."""
        flags = []
        for r in self.records.values():
            bits = _bits(r.buf)
            flags += [(bits[:r.lo] != r.guard_fill).any(), (bits[r.lo + r.n:] != r.guard_fill).any()]
        for name in self._names("output", outputs):
            r = self.records[name]
            flags.append((_bits(r.view) == r.fill).any())
            if r.view.dtype == torch.float32:
                flags.append((~torch.isfinite(r.view)).any())
        for name in self._names("input", inputs):
            r = self.records[name]
            flags.append((_bits(r.view) != r.snapshot).any())
        return bool(torch.stack(flags).any()) if flags else False

    def verify(self, outputs=None, scratch=None, inputs=None):
        """outputs / scratch / inputs: names to check as such (None: every buffer recorded as that kind; a recorded output
        that the call was told not to write -- an optional one passed as NULL -- is simply not listed).  Guards are checked
        for every recorded buffer whatever the lists say."""
        if not self._suspect(outputs, inputs):               # one device synchronisation when everything is in order
            self._names("scratch", scratch)
            return len(self.records)
        for r in self.records.values():
            bits = _bits(r.buf)
            before, after = bits[:r.lo] != r.guard_fill, bits[r.lo + r.n:] != r.guard_fill
            if bool(before.any()):
                raise AssertionError(f"{r.name}: guard before the {r.kind} written at offset {_first(before) - r.lo}")
            if bool(after.any()):
                raise AssertionError(f"{r.name}: guard after the {r.kind} written at offset {r.n + _first(after)} "
                                     f"(the view has {r.n} elements)")
        for name in self._names("output", outputs):
            r = self.records[name]
            flat = r.view.reshape(-1)
            unwritten = _bits(flat) == r.fill
            if bool(unwritten.any()):
                raise AssertionError(f"{name}: output element at offset {_first(unwritten)} of {r.n} still carries the fill "
                                     f"({int(unwritten.sum())} unwritten)")
            if flat.dtype == torch.float32:
                bad = ~torch.isfinite(flat)
                if bool(bad.any()):
                    raise AssertionError(f"{name}: output element at offset {_first(bad)} of {r.n} is not finite "
                                         f"({float(flat[_first(bad)])})")
        self._names("scratch", scratch)
        for name in self._names("input", inputs):
            r = self.records[name]
            changed = _bits(r.view).reshape(-1) != r.snapshot.reshape(-1)
            if bool(changed.any()):
                raise AssertionError(f"{name}: input modified at offset {_first(changed)} of {r.n}")
        return len(self.records)


# ---- the header ---------------------------------------------------------------------------------------------------------
def prototypes(text):
    """include/dfgnn.h -> {entry: [(C type, parameter name), ...]} for every dfgnn_* function it declares; types are
    normalised to one space before a '*' ("const float *", "int", "dfgnn_stream_t")."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(dfgnn_\w+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in (params.split(",") if params.strip() != "void" else []):
            m = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, flags=re.S)
            ctype = re.sub(r"\s*\*\s*", " *", " ".join(m.group(1).split())).strip()
            plist.append((ctype, m.group(2)))
        assert name not in out, f"{name} is declared twice"
        out[name] = plist
    return out


def stream_entries(protos):
    """The entries that launch: those whose last parameter is `dfgnn_stream_t stream`."""
    return sorted(n for n, p in protos.items() if p and p[-1] == ("dfgnn_stream_t", "stream"))
