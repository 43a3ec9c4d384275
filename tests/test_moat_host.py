"""The red-zone helper (tests/moat.py) proven on the CPU: tiny torch stand-ins for kernels, one honest and ten with an injected fault,
each of which must be reported with the right buffer, role and byte offset.  (The coverage gate of tests/test_hip_bounds.py — every entry
point of include/satools_hip.h has a row there or is exempt because it launches no kernel — is in tests/test_components_host.py.)"""
import torch

import moat
from moat import Buf, Moat, run_case

R, T = 3, 37


def _x():
    return torch.randn(R, T, generator=torch.Generator().manual_seed(0))


def _specs(extra=()):
    return [Buf("x", "in", (R, T), data=_x()), Buf("y", "out", (R, T))] + list(extra)


def _far(t, off):
    """one element `off` elements from the start of t's buffer, inside or outside it: what a kernel's pointer arithmetic can reach"""
    at = t.storage_offset() + off
    if not 0 <= at < t.untyped_storage().nbytes() // t.element_size():
        return torch.zeros(1, dtype=t.dtype)       # (the plain run: outside a plain tensor's allocation, where a stand-in must not go)
    return t.as_strided((1,), (1,), at)


def honest(t):
    t["y"].copy_(2 * t["x"] + 1)


def _only(v, kind):
    got = [x for x in v if x.kind == kind]
    assert got, [str(x) for x in v]
    return got


def test_honest_function_passes():
    v, m, plain = run_case(_specs(), honest)
    assert v == [], [str(x) for x in v]
    assert torch.equal(m.t["y"], 2 * _x() + 1)
    assert m.np["y"].shape == (R, T) and m.np["y"].ctypes.data == m.t["y"].data_ptr()      # numpy views of the same bytes


def test_layout_zones_alignment_and_fills():
    assert moat.zone_bytes(4) == 1 << 20 and moat.zone_bytes(1 << 20) == 1 << 20
    assert moat.zone_bytes(3 << 20) == 3 << 20 and moat.zone_bytes(200 << 20) == 64 << 20
    specs = _specs([Buf("big", "workspace", (3 << 18,)), Buf("idx", "in", (5,), torch.int32, data=torch.arange(5, dtype=torch.int32), index=True)])
    for fill, byte, iv in (("A", 0xFF, 0), ("B", 0x47, 1)):
        m = Moat(specs, fill)
        for name, sl in m.slots.items():
            assert sl.start % 256 == 0 and sl.zone >= max(1 << 20, min(sl.spec.nbytes, 64 << 20))
            assert (m.t[name].data_ptr() - sl.flat.data_ptr()) == sl.start
        assert (m.t["y"].view(torch.uint8) == byte).all() and (m.t["big"].view(torch.uint8) == byte).all()
        sl = m.slots["idx"]
        around = sl.flat[sl.start - 64:sl.start + 256 + 64].view(torch.int32)
        assert (around[:16] == iv).all() and (around[16 + 5:] == iv).all() and around[16:21].tolist() == [0, 1, 2, 3, 4]
        assert m.check() == []
    a = Moat(specs, "A").t["y"]
    assert torch.isnan(a).all() and torch.isnan(a.view(torch.float16)).all()
    b = Moat(specs, "B").t["y"]
    assert torch.isfinite(b).all() and (b > 5e4).all() and (b.view(torch.float16) < 8).all()


def test_write_one_element_before_the_start():
    def k(t):
        honest(t)
        _far(t["y"], -1)[0] = 5.0
    w = _only(run_case(_specs(), k)[0], "W")
    assert {(x.buf, x.role, x.side, x.first, x.last) for x in w} == {("y", "out", "before", -4, -1)}
    assert {x.fill for x in w} == {"A", "B"}


def test_write_one_element_after_the_end():
    def k(t):
        honest(t)
        _far(t["y"], R * T)[0] = 5.0
    w = _only(run_case(_specs(), k)[0], "W")
    assert {(x.buf, x.role, x.side, x.first, x.last) for x in w} == {("y", "out", "after", R * T * 4, R * T * 4 + 3)}


def test_write_a_whole_row_stride_past_the_end():
    def k(t):
        honest(t)
        _far(t["y"], R * T + T - 1)[0] = 5.0        # column T - 1 of row R
    w = _only(run_case(_specs(), k)[0], "W")
    off = (R * T + T - 1) * 4
    assert {(x.buf, x.role, x.side, x.first, x.last) for x in w} == {("y", "out", "after", off, off + 3)}


def test_write_into_an_untouched_region():
    def k(t):
        honest(t)
        t["g"][1, 2] = 5.0
        t["y2"][0, 0] = 5.0                       # a channel of a strided output the call does not own
    keep = torch.zeros(R, T, dtype=torch.bool)
    keep[0] = True
    v = run_case(_specs([Buf("g", "untouched", (R, T)), Buf("y2", "out", (R, T), untouched=keep)]), lambda t: (k(t), t["y2"][1:].fill_(1.0)))[0]
    w = _only(v, "W")
    off = (T + 2) * 4
    assert {(x.buf, x.role, x.side, x.first, x.last) for x in w} == {("g", "untouched", "inside", off, off + 3), ("y2", "out/untouched", "inside", 0, 3)}
    assert not [x for x in v if x.kind != "W"]


def test_write_into_an_input():
    def k(t):
        honest(t)
        t["x"][2, 5] = 5.0
    v = run_case(_specs(), k)[0]
    off = (2 * T + 5) * 4
    assert {(x.buf, x.role, x.side, x.first, x.last) for x in _only(v, "W")} == {("x", "in", "inside", off, off + 3)}
    assert not [x for x in v if x.kind != "W"]


def test_read_at_x_T_added_into_the_result():
    def k(t):
        honest(t)
        t["y"][-1, -1] += _far(t["x"], R * T)[0]
    v = run_case(_specs(), k)[0]
    ru = _only(v, "R/U")
    off = (R * T - 1) * 4
    assert len(ru) == 1 and (ru[0].buf, ru[0].role) == ("y", "out") and off <= ru[0].first <= ru[0].last <= off + 3
    assert not [x for x in v if x.kind == "W"]


def test_read_through_fmax_needs_both_fills():
    """fmax swallows NaN: under fill A alone the stray read is invisible — the output even has the honest bits.  Fill B (a large finite
    f32) comes through the fmax, and the A / B comparison reports it."""
    def k(t):
        honest(t)
        t["y"][-1, -1] = torch.fmax(t["y"][-1, -1], _far(t["x"], R * T)[0])
    a = Moat(_specs(), "A")
    k(a.t)
    assert a.check() == [] and torch.equal(a.t["y"], 2 * _x() + 1)          # NaN fill alone: passes
    v = run_case(_specs(), k)[0]
    ru = _only(v, "R/U")
    off = (R * T - 1) * 4
    assert len(ru) == 1 and ru[0].buf == "y" and off <= ru[0].first <= ru[0].last <= off + 3


def test_output_element_left_unwritten():
    def k(t):
        y = 2 * t["x"] + 1
        keep = t["y"][1, 5].clone()
        t["y"].copy_(y)
        t["y"][1, 5] = keep
    ru = _only(run_case(_specs(), k)[0], "R/U")
    off = (T + 5) * 4
    assert len(ru) == 1 and (ru[0].buf, ru[0].role, ru[0].side) == ("y", "out", "inside") and off <= ru[0].first <= ru[0].last <= off + 3


def test_workspace_cell_read_before_it_is_written():
    def k(t):
        honest(t)
        t["y"][0] += t["ws"]              # ws[7] is read before anything wrote it
        t["ws"].copy_(t["x"][0])
    def ok(t):
        t["ws"].copy_(t["x"][0])
        honest(t)
        t["y"][0] += t["ws"]
    specs = _specs([Buf("ws", "workspace", (T,))])
    assert run_case(specs, ok)[0] == []
    ru = _only(run_case(specs, k)[0], "R/U")
    assert len(ru) == 1 and ru[0].buf == "y" and 0 <= ru[0].first and ru[0].last < T * 4


def test_index_read_past_the_end():
    """the entry after the last index is a VALID index under both fills (0 / 1): the stray read picks another table row, no wild address"""
    N = 6
    idx = torch.tensor([3, 1, 4, 1, 5, 2], dtype=torch.int32)
    table = torch.arange(10, dtype=torch.float32) * 1.5 + 1
    def k(t, n_read):
        for i in range(N):
            t["y"][i] = t["table"][int(t["idx"][i])]
        if n_read > N:
            t["y"][N - 1] += t["table"][int(_far(t["idx"], N)[0])]
    specs = [Buf("idx", "in", (N,), torch.int32, data=idx, index=True), Buf("table", "in", (10,), data=table), Buf("y", "out", (N,))]
    assert run_case(specs, lambda t: k(t, N))[0] == []
    ru = _only(run_case(specs, lambda t: k(t, N + 1))[0], "R/U")
    assert len(ru) == 1 and ru[0].buf == "y" and (N - 1) * 4 <= ru[0].first <= ru[0].last < N * 4


def test_dont_care_input_pad_must_not_reach_a_result():
    pad = torch.zeros(R, T, dtype=torch.bool)
    pad[:, T - 5:] = True
    specs = [Buf("x", "in", (R, T), data=_x(), dontcare=pad), Buf("y", "out", (R, T), free=pad)]
    def ok(t):
        t["y"][:, :T - 5] = 2 * t["x"][:, :T - 5]
    def leaky(t):
        ok(t)
        t["y"][0, 0] += t["x"][0, T - 5]
    assert run_case(specs, ok)[0] == []
    ru = _only(run_case(specs, leaky)[0], "R/U")
    assert ru[0].buf == "y" and ru[0].first < 4
