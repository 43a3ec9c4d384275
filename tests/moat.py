"""Red zones around every buffer of one kernel call (tests/test_hip_bounds.py; proven on the CPU by tests/test_moat_host.py).

A `Moat` carves every buffer of a call — inputs, outputs, in-outs, workspaces — out of ONE flat uint8 allocation per memory space
(device, host), each on a 256-byte boundary between two guard zones of at least 1 MiB (at least the buffer's own size, capped at
64 MiB, for larger buffers: a store that is off by a whole row or batch stride still lands inside the allocation).  Every byte the call
does not own as an input is a FILL byte: the zones, don't-care input pads, pure outputs, workspaces, regions the call must not write.
A case runs under two fills,
    A = 0xFF  (NaN as f32, f16, e5m2 and e4m3)        B = 0x47  (a large finite f32, 0x47474747 = 5.1e4; a small finite f16, 7.28)
and three properties are checked:
    W    a zone, an untouched byte or a byte of an input changed               (Moat.check)
    R/U  the owned outputs of run A and run B differ bit for bit: a read outside the declared inputs reached a result, an owned
         element was never written, or a workspace / output was read before it was written            (diff_runs)
    E    the owned outputs differ from the same call on plainly allocated tensors                     (Moat.diff_plain)
NaN alone does not do: fmax(x, NaN) = x swallows it, which is why there are two fills (test_moat_host.py shows the case).
Integer index buffers (`index=True`) are surrounded by VALID small indices instead, 0 under A and 1 under B: a stray index read then
changes a result instead of forming a wild address — the test is never the cause of a fault.

What this cannot see: a stray read whose value is masked before it reaches an output, and a write farther away than the zone.
Works on CPU tensors too (`Moat.np` gives numpy views of the same bytes)."""
from dataclasses import dataclass, field

import torch

FILLS = {"A": 0xFF, "B": 0x47}
INDEX_FILL = {"A": 0, "B": 1}
ALIGN = 256
MIN_ZONE = 1 << 20
MAX_ZONE = 64 << 20
ROLES = ("in", "out", "inout", "workspace", "untouched")


@dataclass
class Buf:
    """one buffer of a call.  `data`: CPU tensor of `shape` (roles in / inout).  Masks are boolean CPU tensors of `shape`:
    `dontcare`  input elements the ABI lets hold anything (pad columns, unused channels of a strided view): filled, must not reach a result
    `untouched` elements the call must not write (W)
    `free`      output elements nobody reads: neither owned nor guarded.
    Everything else of an out / inout buffer is OWNED output, ABI pad slots a consumer reads included.
    `host`: lives in host memory whatever the Moat's device (index lists the entry point copies itself)."""
    name: str
    role: str
    shape: tuple
    dtype: torch.dtype = torch.float32
    data: torch.Tensor = None
    dontcare: torch.Tensor = None
    untouched: torch.Tensor = None
    free: torch.Tensor = None
    index: bool = False
    host: bool = False

    def __post_init__(self):
        assert self.role in ROLES, self.role
        self.shape = tuple(int(s) for s in self.shape)
        if self.role in ("in", "inout"):
            assert self.data is not None and tuple(self.data.shape) == self.shape and self.data.dtype == self.dtype, self.name
        for m in (self.dontcare, self.untouched, self.free):
            assert m is None or (m.dtype == torch.bool and tuple(m.shape) == self.shape), self.name

    @property
    def nbytes(self):
        n = torch.empty(0, dtype=self.dtype).element_size()
        for s in self.shape:
            n *= s
        return n


@dataclass
class Violation:
    kind: str        # "W", "R/U" or "E"
    buf: str
    role: str
    side: str        # "before", "after" or "inside"
    first: int       # byte offsets from the buffer's start (negative: before it; >= its size: after it)
    last: int
    fill: str = ""

    def __str__(self):
        return f"{self.kind}[{self.fill}] {self.buf} ({self.role}) {self.side}: bytes {self.first}..{self.last}"


def zone_bytes(nbytes):
    z = MIN_ZONE if nbytes <= MIN_ZONE else min(nbytes, MAX_ZONE)
    return (z + ALIGN - 1) // ALIGN * ALIGN


def _span(bad, base=0):
    """first / last index of the True entries of a flat bool tensor, or None"""
    if not bool(bad.any()):
        return None
    nz = bad.nonzero()
    return int(nz[0]) + base, int(nz[-1]) + base


@dataclass
class _Slot:
    spec: Buf
    flat: torch.Tensor
    start: int
    zone: int
    pristine: torch.Tensor = None
    extra: dict = field(default_factory=dict)


class Moat:
    def __init__(self, specs, fill, device="cpu"):
        assert fill in FILLS
        self.fill, self.byte, self.device = fill, FILLS[fill], torch.device(device)
        self.slots, self.t = {}, {}
        for host in (False, True):
            group = [s for s in specs if bool(s.host) == host]
            if not group:
                continue
            off, layout = 0, []
            for s in group:
                z = zone_bytes(s.nbytes)
                size = (max(s.nbytes, 1) + ALIGN - 1) // ALIGN * ALIGN
                layout.append((s, off + z, z))
                off += z + size + z
            flat = torch.full((off,), self.byte, dtype=torch.uint8, device="cpu" if host else self.device)
            assert flat.data_ptr() % ALIGN == 0 or flat.device.type == "cpu"
            # (a CPU allocation is 64-byte aligned: alignment is not under test there)
            for s, start, z in layout:
                assert s.name not in self.slots, s.name
                slot = _Slot(s, flat, start, z)
                self.slots[s.name] = slot
                t = flat[start:start + s.nbytes].view(s.dtype).view(s.shape)
                self.t[s.name] = t
                if s.index:       # valid small indices all around
                    whole = flat[start - z:start + (max(s.nbytes, 1) + ALIGN - 1) // ALIGN * ALIGN + z].view(s.dtype)
                    whole.fill_(INDEX_FILL[fill])
                if s.role in ("in", "inout"):
                    t.copy_(s.data)
                    if s.dontcare is not None:
                        self._fill_where(t, s, s.dontcare.to(t.device))
                if s.untouched is not None or s.role in ("untouched", "in"):
                    slot.pristine = t.clone()          # (an input is nothing the call may write either, its don't-care pads included)

    def _fill_where(self, t, s, mask):
        if s.index:
            t[mask] = INDEX_FILL[self.fill]
        else:
            t.view(torch.uint8).view(*s.shape, t.element_size())[mask] = self.byte

    @property
    def np(self):
        return {k: v.numpy() for k, v in self.t.items() if v.device.type == "cpu"}

    def _zone_expected(self, s, zone):
        if s.index:
            return zone.view(s.dtype) != INDEX_FILL[self.fill], torch.empty(0, dtype=s.dtype).element_size()
        return zone != self.byte, 1

    def check(self):
        """W violations of this run: guard zones, untouched regions and inputs"""
        out = []
        for name, sl in self.slots.items():
            s = sl.spec
            end = sl.start + (max(s.nbytes, 1) + ALIGN - 1) // ALIGN * ALIGN
            for side, lo, hi in (("before", sl.start - sl.zone, sl.start), ("after", sl.start + s.nbytes, end + sl.zone)):
                zone = sl.flat[lo:hi]
                bad, w = self._zone_expected(s, zone)
                sp = _span(bad.reshape(-1))
                if sp:
                    out.append(Violation("W", name, s.role, side, lo - sl.start + sp[0] * w, lo - sl.start + sp[1] * w + w - 1, self.fill))
            if sl.pristine is not None:
                t = self.t[name]
                bad = t.view(torch.uint8).view(*s.shape, t.element_size()) != sl.pristine.view(torch.uint8).view(*s.shape, t.element_size())
                if s.role not in ("untouched", "in"):
                    bad = bad & s.untouched.to(bad.device).unsqueeze(-1)
                sp = _span(bad.reshape(-1))
                if sp:
                    out.append(Violation("W", name, s.role if s.role in ("untouched", "in") else s.role + "/untouched", "inside", sp[0], sp[1], self.fill))
        return out

    def owned(self, name):
        """bool mask [*shape] of the owned output elements of an out / inout buffer"""
        s = self.slots[name].spec
        m = torch.ones(s.shape, dtype=torch.bool)
        for x in (s.untouched, s.free):
            if x is not None:
                m &= ~x
        return m

    def outputs(self):
        return [n for n, sl in self.slots.items() if sl.spec.role in ("out", "inout")]

    def _diff(self, name, other, kind, tol=None):
        s = self.slots[name].spec
        a, b = self.t[name], other
        own = self.owned(name).to(a.device)
        if tol is not None and a.dtype.is_floating_point:
            bad = ~((a.double() - b.double()).abs() <= tol) & ~(torch.isnan(a) & torch.isnan(b))
            bad = (bad & own).unsqueeze(-1).expand(*s.shape, a.element_size())
        else:
            e = a.element_size()
            bad = (a.view(torch.uint8).view(*s.shape, e) != b.contiguous().view(torch.uint8).view(*s.shape, e)) & own.unsqueeze(-1)
        sp = _span(bad.reshape(-1))
        return [Violation(kind, name, s.role, "inside", sp[0], sp[1], self.fill)] if sp else []

    def diff_plain(self, plain, tol=None):
        """E: owned outputs against the same call on plainly allocated tensors (`plain`: name -> tensor)"""
        out = []
        for n in self.outputs():
            out += self._diff(n, plain[n].to(self.t[n].device), "E", tol)
        return out


def diff_runs(a, b, tol=None):
    """R / U: the owned outputs of the two fills must have the same bits"""
    out = []
    for n in a.outputs():
        out += a._diff(n, b.t[n], "R/U", tol)
    return out


def plain_tensors(specs, device="cpu"):
    """the same buffers as ordinary allocations: inputs copied (don't-care pads zero), everything else zero"""
    t = {}
    for s in specs:
        dev = "cpu" if s.host else device
        if s.role in ("in", "inout"):
            x = s.data.clone()
            if s.dontcare is not None:
                x[s.dontcare] = 0
            t[s.name] = x.to(dev)
        else:
            t[s.name] = torch.zeros(s.shape, dtype=s.dtype, device=dev)
    return t


def run_case(specs, call, device="cpu", tol=None, sync=None):
    """the whole protocol for one case: `call(tensors)` under fill A, fill B and on plain tensors.  Returns (violations, moat A, plain)"""
    v, moats = [], []
    for fill in ("A", "B"):
        m = Moat(specs, fill, device)
        call(m.t)
        if sync:
            sync()
        v += m.check()
        moats.append(m)
    v += diff_runs(moats[0], moats[1], tol)
    plain = plain_tensors(specs, device)
    call(plain)
    if sync:
        sync()
    v += moats[0].diff_plain(plain, tol)
    return v, moats[0], plain
