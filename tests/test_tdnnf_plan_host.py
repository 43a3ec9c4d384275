"""The TDNNF stack's host path, CPU only: the sequence of C-ABI calls and every descriptor in it against a recorded trace, and the
soundness of the per-layer plan that drives them.

`ops.lib` is replaced by a recorder (every `sat_*` call returns 0 and is logged), `ops.ptr` by a function that hands out the
`data_ptr()` of CPU tensors and keeps each alive for the run (no address is reused), `ops.stream` by a constant; the library itself
is only loaded by `packing`.  A logged call holds the entry name, every scalar argument and descriptor field (floats as hex) and
every pointer as NULL or "b<k>+<byte offset>", buffers numbered by the first appearance of their storage — so the log pins shapes,
modes, strides, `no_y`, NULL `x` / `y`, which planes feed which call, and aliasing.

tests/golden/tdnnf_call_trace.json holds the expected logs: one summary line and the SHA-1 of the full record per call.  It was
recorded by running this module as a script (`python tests/test_tdnnf_plan_host.py`) on the commit BEFORE the per-layer plan
replaced `_tdnnf_layer`'s branch cascade (the methods driven have the same names there), and is not to be re-recorded to make a
host-side change pass: a difference is a change of what is launched."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import satools_amd  # noqa: E402,F401
from satools_amd import _lib, asrbn, ops, wav2vec2  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "tdnnf_call_trace.json")
STREAM = 0x57AE
SETTINGS = [("f16x3", True), ("f16x3", False), ("f32", True), ("f32", False)]

# what a summary line shows of a descriptor (the SHA-1 covers every field)
_SHOW = {"ConvDesc": ("B", "C_in", "T_in", "C_out", "T_q", "ksize", "stride", "mode", "no_y", "res_toff", "res_tstride", "bias", "res",
                      "x_split", "y_split"),
         "TdnnfLayerDesc": ("B", "feat_dim", "bottleneck_dim", "out_dim", "T_in", "context_len", "mode", "bypass_scale", "x", "x_split", "y",
                            "y_split", "z", "z_split")}


class Recorder:
    """stands in for the library (`sat_*` attributes), `ops.ptr` and `ops.stream`"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.calls, self.keep, self.spans, self.names = [], [], {}, {}

    def ptr(self, t, strided=False):
        if t is None:
            return None
        if (t.stride(-1) != 1) if strided else (not t.is_contiguous()):
            raise _lib.SatError("HIP entry points need contiguous tensors")
        st = t.untyped_storage()
        self.keep.append(t)
        self.spans[st.data_ptr()] = st.nbytes()
        return t.data_ptr()

    def _where(self, addr):
        if not addr:
            return "NULL"
        if addr == STREAM:
            return "stream"
        for base, n in self.spans.items():
            if base <= addr < base + n:
                return f"b{self.names.setdefault(base, len(self.names))}+{addr - base}"
        raise AssertionError(f"pointer {addr:#x} lies in no tensor handed to ops.ptr")

    def _value(self, ctype, v):
        if ctype is C.c_void_p:
            return self._where(v)
        if ctype is C.c_float:
            return C.c_float(v).value.hex()
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer) and issubclass(ctype._type_, C.Structure):
            d = v._obj
            return {"struct": type(d).__name__, "fields": [[n, self._value(t, getattr(d, n))] for n, t in d._fields_]}
        return int(v)

    def __getattr__(self, name):
        if not name.startswith("sat_"):
            raise AttributeError(name)
        argtypes = _lib.COMPONENTS["core"][name][1]

        def call(*args):
            assert len(args) == len(argtypes), name
            self.calls.append([name, [self._value(t, a) for t, a in zip(argtypes, args)]])
            return 0
        return call

    def lines(self):
        """[summary, SHA-1 of the full record] per call"""
        out = []
        for name, args in self.calls:
            parts = [name]
            for a in args:
                if isinstance(a, dict):
                    parts.append("{" + " ".join(f"{n}={v}" for n, v in a["fields"] if n in _SHOW[a["struct"]]) + "}")
                else:
                    parts.append(str(a))
            out.append([" ".join(parts), hashlib.sha1(json.dumps([name, args]).encode()).hexdigest()])
        return out


@pytest.fixture()
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "lib", lambda: r)
    monkeypatch.setattr(ops, "ptr", r.ptr)
    monkeypatch.setattr(ops, "stream", lambda: STREAM)
    return r


SMALL = {"small64": dict(hidden_dim=64, bottleneck_dim=16, prefinal_bottleneck_dim=32, kernel_size_list=([3, 2, 1, 5, 3, 1, 3], [1, 3]),
                         subsampling_factor_list=([1, 1, 3, 1, 2, 2, 1], [1.5, 1]), codebook_size=100),
         "small72": dict(hidden_dim=72, bottleneck_dim=24, prefinal_bottleneck_dim=40, kernel_size_list=([3, 1, 3, 3], [1, 3]),
                         subsampling_factor_list=([1, 2, 1, 1], [1.5, 1]), codebook_size=48)}
ARCHS = ["fbank_vq", "fbank", "w2v2_vq", "w2v2", "small64", "small72"]


def build_net(arch):
    """-> (net, input channels, frames, drive forward_ragged?)"""
    if arch.startswith("w2v2"):
        full = wav2vec2.Wav2Vec2Params
        wav2vec2.Wav2Vec2Params = lambda n_layers=24: full(1)        # the encoder is never driven
        try:
            net = (wav2vec2.TdnnfWav2vec2VqNet if arch == "w2v2_vq" else wav2vec2.TdnnfWav2vec2Net)(output_dim=8)
        finally:
            wav2vec2.Wav2Vec2Params = full
        c_in, T, ragged = 1024, 60, False
    else:
        net = asrbn.TdnnfNet(output_dim=8) if arch == "fbank" else asrbn.TdnnfVqNet(output_dim=8, **SMALL.get(arch, {}))
        c_in, T, ragged = 80, 120, True
    net.vq_tie_sigmas = 0
    return net.eval(), c_in, T, ragged


def drive(rec, net, c_in, T, ragged):
    """the logs of the driven methods of `net` as it is set: {run: lines}"""
    out = {}

    def run(name, f):
        rec.reset()
        with torch.no_grad():
            f()
        out[name] = rec.lines()
    n_codes = net._stack_layers()[-1].bottleneck_func.quant._embedding.weight.shape[0] if net._has_vq() else 1
    tie = asrbn._TieCtx(torch.zeros(n_codes, n_codes), 0.5, torch.zeros(3, 2, dtype=torch.int32))
    run("run_stack", lambda: net._run_stack(torch.zeros(2, c_in, T), want_aux=True))
    run("run_stack_tie", lambda: net._run_stack(torch.zeros(2, c_in, T), want_aux=True, tie=tie))
    run("asr_outputs", lambda: net._asr_outputs(torch.zeros(2, c_in, T)))
    if ragged:
        run("forward_ragged", lambda: net.forward_ragged([torch.zeros(16000), torch.zeros(1, 24000)]))
    rec.reset()
    return out


def set_arith(net, precision, planes_only):
    net.precision, net.tdnnf_planes_only = precision, planes_only


def trace_all(rec):
    """every architecture as ONE live net whose attributes are flipped through SETTINGS -> {"arch/precision/planes<0|1>/run": lines}"""
    logs = {}
    for arch in ARCHS:
        net, *how = build_net(arch)
        for precision, planes_only in SETTINGS:
            set_arith(net, precision, planes_only)
            for name, lines in drive(rec, net, *how).items():
                logs[f"{arch}/{precision}/planes{int(planes_only)}/{name}"] = lines
    return logs


def load_fixture():
    fx = json.load(open(FIXTURE))
    return {k: fx["logs"][i] for k, i in fx["runs"].items()}


def assert_same_log(key, got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{key}: call {i} differs\n  now      {g[0]}\n  recorded {w[0]}" + ("" if g[0] != w[0] else "\n  (a field the summary does not show)")
    assert len(got) == len(want), f"{key}: {len(got)} calls, recorded {len(want)}; first surplus: {(got + want)[min(len(got), len(want))][0]}"


@pytest.fixture(scope="module")
def traced():
    """(logs of every live net, the nets): built once for the module"""
    mp = pytest.MonkeyPatch()
    r = Recorder()
    mp.setattr(ops, "lib", lambda: r)
    mp.setattr(ops, "ptr", r.ptr)
    mp.setattr(ops, "stream", lambda: STREAM)
    try:
        logs, nets = {}, {}
        for arch in ARCHS:
            net, *how = nets[arch] = build_net(arch)
            # (the first setting comes round again at the end: a memoised plan must survive the flips in between)
            for precision, planes_only in SETTINGS + SETTINGS[:1]:
                set_arith(net, precision, planes_only)
                for name, lines in drive(r, net, *how).items():
                    logs.setdefault(f"{arch}/{precision}/planes{int(planes_only)}/{name}", []).append(lines)
    finally:
        mp.undo()
    return logs, nets


def test_call_trace_equals_the_recorded_one(traced):
    """every call of every driven method, in order, field for field: a call added, dropped or reordered, or any changed scalar,
    stride or pointer role fails here and names the call"""
    logs, _ = traced
    want = load_fixture()
    assert sorted(logs) == sorted(want)
    for key, visits in logs.items():
        for got in visits:
            assert_same_log(key, got, want[key])


def test_trace_reaches_every_live_form():
    """the fixture itself: the one-call layer on planes with x = y = NULL, the 1.5x unfold layer, both context-free subsampling
    forms (planes: an act_split behind a 1x1 product; gathered), strided f32, and both VQ entries with and without the tie count"""
    want = load_fixture()
    names = {ln[0].split()[0] for lines in want.values() for ln in lines}
    assert {"sat_tdnnf_layer_f32", "sat_conv1d_f32", "sat_tdnnf_unfold15_f32", "sat_act_split_f32", "sat_vq_argmin_gather_f32",
            "sat_vq_argmin_gather_tie_f32", "sat_vq_argmin_gather_tiled_f32", "sat_vq_argmin_gather_tiled_tie_f32", "sat_pad_replicate_f32",
            "sat_log_softmax_channels_f32", "sat_fbank_cmvn_pad_f32"} <= names
    on = [ln[0] for ln in want["fbank_vq/f16x3/planes1/run_stack"] if ln[0].startswith("sat_tdnnf_layer_f32")]
    off = [ln[0] for ln in want["fbank_vq/f16x3/planes0/run_stack"] if ln[0].startswith("sat_tdnnf_layer_f32")]
    assert any(" x=NULL " in s and " y=NULL " in s for s in on) and not any(" x=NULL " in s or " y=NULL " in s for s in off)
    assert any("stride=2" in ln[0] for ln in want["small64/f16x3/planes1/run_stack"])


def test_fresh_net_under_a_setting_gives_the_flipped_nets_log(rec):
    """flipping `precision` / `tdnnf_planes_only` on a live net (test_call_trace_equals_the_recorded_one) gives the log of a net
    BUILT under that setting: nothing planned under another setting is carried over"""
    want = load_fixture()
    for arch in SMALL:
        for precision, planes_only in SETTINGS:
            net, *how = build_net(arch)
            set_arith(net, precision, planes_only)
            for name, lines in drive(rec, net, *how).items():
                assert_same_log(f"{arch}/{precision}/planes{int(planes_only)}/{name}", lines, want[f"{arch}/{precision}/planes{int(planes_only)}/{name}"])


def _plans(net, precision, planes_only):
    set_arith(net, precision, planes_only)
    net._prepare_full(torch.device("cpu"))
    return net._planned(False), net._planned(True)


def test_plan_skips_an_f32_store_only_before_a_layer_that_does_not_read_it(traced):
    _, nets = traced
    skipped = {}
    for arch, (net, *_) in nets.items():
        for precision, planes_only in SETTINGS:
            stack, through = _plans(net, precision, planes_only)
            assert len(stack) == len(net._stack_layers())
            skipped[arch, precision, planes_only] = sum(p.skip_f32 for _, _, p in stack)
            for i, (_, _, p) in enumerate(stack):
                if p.skip_f32:
                    nxt = stack[i + 1][2]
                    assert planes_only and precision == "f16x3" and p.form == "one_call" and p.planes_out
                    assert not nxt.reads_f32 and nxt.planes_in and nxt.x_unwritten
                else:
                    assert i + 1 == len(stack) or not stack[i + 1][2].x_unwritten
            # the runs through every layer never skip a store
            for run in [through["stack"], through["after"]] + through["prefinal"]:
                assert not any(p.skip_f32 or p.x_unwritten or p.bottleneck_only for _, _, p in run)
            assert stack[-1][2].bottleneck_only and not any(p.bottleneck_only for _, _, p in stack[:-1])
    # the fbank stack: every plain layer but the one in front of the subsampling layer (its strided bypass reads f32); the wav2vec2 tail: the
    # layer in front of the bottleneck (tdnn1 takes its bypass from the f32 features); small72: no channel count is a multiple of 16
    want = {"fbank_vq": 9, "fbank": 9, "w2v2_vq": 1, "w2v2": 1, "small64": 1, "small72": 0}
    assert skipped == {(a, pr, po): (n if pr == "f16x3" and po else 0) for a, n in want.items() for pr, po in SETTINGS}


def test_plan_is_memoised_per_cache_list_and_setting(traced):
    _, nets = traced
    net = nets["small64"][0]
    a = _plans(net, "f16x3", True)
    assert _plans(net, "f16x3", True)[0] is a[0] and _plans(net, "f16x3", True)[1] is a[1]
    b = _plans(net, "f16x3", False)
    assert b[0] is not a[0] and [p for *_, p in b[0]] != [p for *_, p in a[0]]
    c = _plans(net, "f32", True)
    assert all(p.form in ("two_call", "one_call") and not p.planes_in and not p.skip_f32 for *_, p in c[0])
    assert _plans(net, "f16x3", True)[0] is a[0]
    assert len(net.__dict__["_plans"]) <= 8


def test_inconsistent_plan_is_refused_before_any_launch(rec):
    """a layer that skips its f32 store in front of one that reads it (here: a subsampling layer whose strided bypass reads f32) is
    an error when the plan is built or checked, not an assert in the middle of a forward pass"""
    net, c_in, T, _ = build_net("small64")
    set_arith(net, "f16x3", True)
    net._prepare(torch.device("cpu"))
    layers, caches = net._stack_layers(), net._cache
    plan = asrbn.plan_layers(layers, caches, True, True)
    assert plan[1].skip_f32 is False and plan[2].form == "sub_planes" and plan[2].reads_f32     # ctx 1, sub 3, with bypass
    bad = list(plan)
    bad[1] = bad[1]._replace(skip_f32=True)
    with pytest.raises(_lib.SatError, match="reads"):
        asrbn.check_plan(bad)
    bad[2] = bad[2]._replace(x_unwritten=True)
    with pytest.raises(_lib.SatError, match="reads"):
        asrbn.check_plan(bad)
    last = list(plan)
    last[-1] = last[-1]._replace(skip_f32=True)
    with pytest.raises(_lib.SatError):
        asrbn.check_plan(last)
    # a 1.5x layer cannot hand back its bottleneck: refused when planned (it was an assert inside the forward pass)
    head = [m for m in net.tdnnfs_after if isinstance(m, asrbn.TDNNFBatchNormParams)]
    net._prepare_full(torch.device("cpu"))
    with pytest.raises(_lib.SatError, match="1.5"):
        asrbn.plan_layers(head[:1], [net._cache_full["after"][0][1]], True, True)
    assert rec.calls == []


def test_fbank_mel_ranges_are_those_of_ops():
    """`_fbank_tables` takes lo / hi from ops.mel_filter_ranges: the int32 values of the formula it used to carry"""
    mel = asrbn.mel_banks(80)
    nz = mel > 0
    lo = torch.where(nz.any(1), nz.float().argmax(1), torch.zeros(mel.shape[0], dtype=torch.long))
    hi = mel.shape[1] - torch.flip(nz, [1]).float().argmax(1)
    hi = torch.where(nz.any(1), hi, torch.zeros_like(hi))
    got = ops.mel_filter_ranges(mel)
    assert got[0].dtype == got[1].dtype == torch.int32
    assert torch.equal(got[0], lo.to(torch.int32)) and torch.equal(got[1], hi.to(torch.int32))
    win, mel_t, lo_t, hi_t = asrbn.TdnnfVqNet(output_dim=8, **SMALL["small72"])._fbank_tables(torch.device("cpu"))
    assert torch.equal(lo_t, got[0]) and torch.equal(hi_t, got[1]) and torch.equal(mel_t, mel)


if __name__ == "__main__":
    mp = pytest.MonkeyPatch()
    r = Recorder()
    mp.setattr(ops, "lib", lambda: r)
    mp.setattr(ops, "ptr", r.ptr)
    mp.setattr(ops, "stream", lambda: STREAM)
    logs = trace_all(r)
    mp.undo()
    uniq, runs = [], {}
    for k, lines in logs.items():
        if lines not in uniq:
            uniq.append(lines)
        runs[k] = uniq.index(lines)
    with open(FIXTURE, "w") as f:
        f.write('{"runs": ' + json.dumps(runs, indent=0) + ',\n"logs": [\n' +
                ",\n".join("[\n" + ",\n".join(json.dumps(ln) for ln in lines) + "\n]" for lines in uniq) + "\n]}\n")
    print(f"{len(runs)} runs, {len(uniq)} distinct logs, {sum(len(u) for u in uniq)} calls -> {FIXTURE}")
